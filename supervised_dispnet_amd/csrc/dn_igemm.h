// What the two tiled implicit-GEMM files (dn_tiled.hip, dn_tiled_wgrad.hip) share: the generic K-group gather of the A operand and the
// launchers' dynamic-LDS opt-in.  Not part of the ABI.
#pragma once
#include "dn_device.h"

namespace dn {

// One 4-wide K group of one row of the A operand.
struct AGroup {
  f32x4 v;
  bool ok;     // vector path: halo / tail predicate (value must be zeroed after the deferred affine)
};

// Gathers 4 consecutive K elements [kl, kl+4) of operand S for the pixel context (n, by, bx).
// Vector path: one 16-byte load, affine deferred to the caller (returns raw value + predicate).
// Scalar path: element-wise, fully resolved here (affine applied, zeros filled); ok = true, *defer = false.
__device__ __forceinline__ AGroup gather4(const KOperand& S, int kl, int ntaps, const int* taps, int n, int by, int bx,
                                          bool rowvalid, int IH, int IW, int j_vec, int c_vec, int reflect) {
  AGroup r;
  r.v = f32x4{0.f, 0.f, 0.f, 0.f};
  r.ok = false;
  if (S.vec) {
    if (rowvalid && j_vec < ntaps) {
      int t = taps[j_vec];
      int iy = by + (int)(short)(t & 0xffff), ix = bx + (t >> 16);
      if (reflect) {
        iy = reflect_idx(iy, IH);
        ix = reflect_idx(ix, IW);
      }
      if ((unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW) {
        const float* a = S.p + n * S.sn + (long long)(iy >> S.up) * S.sh + (long long)(ix >> S.up) * S.sw + c_vec;
        r.v = *reinterpret_cast<const f32x4*>(a);
        r.ok = true;
      }
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      int k = kl + e;
      int j = k / S.C, c = k - j * S.C;
      float val = 0.f;
      if (rowvalid && j < ntaps) {
        int t = taps[j];
        int iy = by + (int)(short)(t & 0xffff), ix = bx + (t >> 16);
        if (reflect) {
          iy = reflect_idx(iy, IH);
          ix = reflect_idx(ix, IW);
        }
        if ((unsigned)iy < (unsigned)IH && (unsigned)ix < (unsigned)IW) {
          val = S.p[n * S.sn + (long long)(iy >> S.up) * S.sh + (long long)(ix >> S.up) * S.sw + (long long)c * S.sc];
          if (S.scale) val = fmaxf(0.f, val * S.scale[c] + S.shift[c]);
        }
      }
      r.v[e] = val;
    }
    r.ok = true;
  }
  return r;
}

template <typename K>
static int enable_big_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return DN_OK;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) {
    set_error("hipFuncSetAttribute(max dynamic LDS %zu): %s", bytes, hipGetErrorString(e));
    return DN_ERR_LAUNCH;
  }
  return DN_OK;
}

}  // namespace dn
