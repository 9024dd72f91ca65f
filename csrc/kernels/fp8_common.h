// e4m3 MFMA operand helpers shared by the fp8 conv2 kernels (cnn_fp8.hip) and the fp8 variant of the
// whole-network inference launch (cnn_infer.hip).
#pragma once
#include "conv_common.h"

namespace dmlc {

typedef int fp8x32 __attribute__((ext_vector_type(8)));   // 32 packed e4m3 values (MFMA operand)

constexpr int X8_BYTES = 256 * 64;            // [16x16 padded pixels][64 ch] fp8

// 16-B unit u (16 channels) of padded pixel P: the units are XOR-swizzled by the padded row's parity
DEV int x8_addr(int P, int u) { return P * 64 + ((u ^ ((P >> 4) & 1)) << 4); }

DEV f32x4 mfma_fp8(const fp8x32& a, const fp8x32& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}
DEV fp8x32 lds_fp8x32(const uint8_t* lo, const uint8_t* hi) {
  const uint4 a = *reinterpret_cast<const uint4*>(lo), b = *reinterpret_cast<const uint4*>(hi);
  const fp8x32 r = {(int)a.x, (int)a.y, (int)a.z, (int)a.w, (int)b.x, (int)b.y, (int)b.z, (int)b.w};
  return r;
}

}  // namespace dmlc
