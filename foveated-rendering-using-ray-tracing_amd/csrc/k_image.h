// k_image.h — what the image-space stages share across translation units: the JumpFlooding state encoding
// (k_jfa.hip writes it, k_sibson.hip reads the seeds from it) and the prefix-sum block count both launchers use.
#pragma once
#include "fr_device.h"

namespace fr {

// JumpFlooding state words (the layout is described at the head of k_jfa.hip)
#define JFA_FLAG 0x80000000u
#define JFA_UNSEEDED 0x7F800000u  // +inf in .x

FR_DEV f2 frag_uv(uint32_t x, uint32_t y, f2 screen) { return mk2(((float)x + 0.5f) / screen.x, ((float)y + 0.5f) / screen.y); }
FR_DEV float jfa_coord(uint32_t w) { return fabsf(__uint_as_float(w)); }  // coordinates are > 0: |x| clears the flag
FR_DEV bool jfa_seeded(uint32_t wx) { return wx != JFA_UNSEEDED; }

int sibson_prefix_blocks(int W);  // k_sibson.hip: 64-column blocks of a row's W + 1 prefix sums

}  // namespace fr
