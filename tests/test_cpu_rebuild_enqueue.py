"""CPU suite for the stream-ordered rebuild (fr_rebuild_bvh_enqueue, fr_bvh_rebuild_status): what can be said of
the two calls without a device. The GPU suite is test_gpu_rebuild_enqueue.py."""
import ctypes as C

NAMES = ("fr_rebuild_bvh_enqueue", "fr_bvh_rebuild_status")


def test_library_exports_both_calls(fovrt_mod):
    lib = fovrt_mod.load_library()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in fovrt_mod._SIGS, name  # (test_cpu_abi then demands them of the header)


def test_null_context_is_invalid_without_a_device(fovrt_mod):
    lib = fovrt_mod.load_library()
    assert lib.fr_rebuild_bvh_enqueue(None) == fovrt_mod.FR_E_INVALID
    b, f = C.c_uint64(7), C.c_uint64(7)
    assert lib.fr_bvh_rebuild_status(None, C.byref(b), C.byref(f)) == fovrt_mod.FR_E_INVALID
    assert lib.fr_bvh_rebuild_status(None, None, None) == fovrt_mod.FR_E_INVALID
    assert (b.value, f.value) == (7, 7)


def test_python_facade_has_both_methods(fovrt_mod):
    for name in ("rebuild_bvh_enqueue", "bvh_rebuild_status"):
        assert callable(getattr(fovrt_mod.PathTracer, name, None)), name
