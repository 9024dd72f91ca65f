// Small helpers shared by the fp32 conv2 code of k_cnn_infer_f32 (f32_infer.hip) and k_f32_conv2
// (f32_conv.hip): the fp32 MFMA, 16-byte LDS reads, the swizzled zero-padded [16][16][64] fp32 LDS image p1
// and the 4x4 pixel tiles of the 12x12 output.  Lane map: see f32_infer.hip.
#pragma once
#include "common.h"

namespace dmlc {

DEV f32x4 mfma_f32(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
DEV f32x4 lds4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
// float offset in p1 of channel chunk c (4 floats) of padded pixel (py, px)
DEV int p1_off(int py, int px, int c) { return (py * 16 + px) * 64 + ((c ^ ((px & 3) | ((py & 3) << 2))) << 2); }
// float offset of conv2 pixel tile t (a 4x4 block of the 12x12 output) in p1 / its first output pixel
constexpr int p1_tile(int t) { return ((t / 3) * 4 * 16 + (t % 3) * 4) * 64; }
constexpr int out_tile(int t) { return (t / 3) * 4 * 12 + (t % 3) * 4; }

}  // namespace dmlc
