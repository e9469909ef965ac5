"""The tables of state_sequence_cases.py, held without a device: deterministic, complete, and the walks meeting the
pairs they must meet. The GPU side (test_gpu_state_sequences.py) runs exactly these lists."""
import numpy as np

import state_sequence_cases as sc
from helpers import ASSET_DIR, TEXTURE_MODE


def test_tables_are_deterministic():
    assert sc.build_matrix() == sc.MATRIX == sc.build_matrix()
    assert [(s,) + sc.walk(s) for s in sc.WALK_SEEDS] == sc.WALKS == [(s,) + sc.walk(s) for s in sc.WALK_SEEDS]
    assert len(set(sc.MATRIX)) == len(sc.MATRIX)


def test_names_are_unique_and_say_how_a_write_was_made():
    names = [s.name for s in sc.PREFIXES + sc.DISTURBERS + sc.OBSERVERS]
    assert len(set(names)) == len(names)
    writes = [d.name for d in sc.DISTURBERS if d.name.startswith("write_")]
    assert all(n.endswith("_own_bytes") or n.endswith("_pattern") for n in writes)
    written = {n[len("write_"):].rsplit("_", 2 if n.endswith("_own_bytes") else 1)[0] for n in writes}
    assert written == {"SHADING", "JFA_COLOR", "JFA_COORD", "HISTORY_CACHE", "DEPTH", "NORMAL", "WEIGHT", "DIFFUSE",
                       "MASK", "EXTRA"}
    assert {n[len("view_"):] for n in names if n.startswith("view_")} == {"JFA_COORD", "JFA_COLOR", "EXTRA", "HISTORY"}
    assert set(sc.HISTORY_MASK_CAMERA) <= {d.name for d in sc.DISTURBERS}


def test_matrix_holds_every_step_and_every_pair_of_the_main_prefixes():
    have = set(sc.MATRIX)
    assert {d for _, d, _ in have} == {d.name for d in sc.DISTURBERS}
    assert {o for _, _, o in have} == {o.name for o in sc.OBSERVERS}
    assert {p for p, _, _ in have} == {p.name for p in sc.PREFIXES}
    for p in sc.MAIN_PREFIXES:
        for d in sc.DISTURBERS:
            for o in sc.OBSERVERS:
                assert (p, d.name, o.name) in have, (p, d, o)
    for p in ("frames_latency", "frames_timed"):
        for d in sc.HISTORY_MASK_CAMERA:
            for o in sc.OBSERVERS:
                assert (p, d, o.name) in have, (p, d, o)
    # the sequence the suite could not see: a restore, then Sibson alone
    for p in sc.MAIN_PREFIXES:
        assert (p, "snapshot_restore", "sibson_alone") in have
        assert (p, "restore_earlier", "sibson_alone") in have
    groups = sc.matrix_groups()
    assert sum(len(v) for v in groups.values()) == len(sc.MATRIX)


def test_refusals_are_listed_and_few():
    assert set(sc.REFUSED) <= set(sc.MATRIX)
    assert len(sc.REFUSED) <= sc.MAX_REFUSED_FRACTION * len(sc.MATRIX)


def test_walks_are_their_seeds_and_meet_the_pairs():
    assert len(sc.WALK_SEEDS) == 16 == len(set(sc.WALK_SEEDS)) and len(sc.WALKS) == 16
    observers = {o.name for o in sc.OBSERVERS}
    steps = observers | {d.name for d in sc.DISTURBERS}
    for seed, prefix, names, knobs in sc.WALKS:
        assert (prefix, names, knobs) == sc.walk(seed)
        assert len(names) == sc.WALK_STEPS == 30 and set(names) <= steps
        assert prefix in {p.name for p in sc.PREFIXES}
        assert 0 < len(knobs) < len(sc.KNOBS) and set(knobs) <= set(sc.KNOBS)  # neither default nor plain
        for i in range(len(names) - 3):
            assert observers & set(names[i:i + 4]), (seed, i, names[i:i + 4])
    met = sc.pairs_met(sc.WALK_SEEDS)
    disturbers = {d.name for d in sc.DISTURBERS}
    assert all(d in disturbers and o in observers for d, o in sc.MUST_MEET)
    assert not set(sc.MUST_MEET) - met, set(sc.MUST_MEET) - met
    assert sc.choose_seeds() == sorted(sc.WALK_SEEDS)  # the seeds are the search's, not picked by hand


def test_moved_model_changes_the_scene_box(fovrt_mod):
    """move_model_refit is there because the scene box changes (an owed EXTRA keeps the box its launch saw)."""
    host = fovrt_mod.Scene(fovrt_mod.Config(width=96, height=64, scene=sc.SCENE, texture_mode=TEXTURE_MODE,
                                            asset_dir=ASSET_DIR))
    a, models = host.arrays(), host.models()
    assert {sc.MOVED_MODEL, sc.HIDDEN_MODEL} <= {m[0] for m in models} and sc.MOVED_MODEL != sc.HIDDEN_MODEL
    moved = sc.moved_positions(a["pos"], models).reshape(-1, 3)
    assert moved.shape[0] * 3 == a["pos"].size and not np.array_equal(moved, a["pos"].reshape(-1, 3))
    assert (moved.max(axis=0) > a["bbox"][3:6]).any() or (moved.min(axis=0) < a["bbox"][0:3]).any()
    rays = sc.ray_batch(fovrt_mod)
    assert rays.dtype == np.float32 and rays.shape[1] == 8
    assert np.allclose(np.linalg.norm(rays[:, 4:7], axis=1), 1.0, atol=1e-6)
