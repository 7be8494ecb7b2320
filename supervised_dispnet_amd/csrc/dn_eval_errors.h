// The per-image selection and sums of the evaluation metrics, shared by dn_eval_errors (dn_eval.hip: the reference's chain, predictions
// clipped before the scale) and dn_eval_errors_clamp (dn_eval_mono2.hip: monodepth2's chain, scale first, clamp last).  One block of
// kErrThreads threads per image over the pixels with mask != 0: numpy's median of gt and of pred by an exact radix select on the bit
// patterns (both arrays per sweep), scale = fp32 ratio, pred * scale rounded to fp32 [then clamped], thresholds from IEEE fp32
// divisions, the four means from fp64 terms and fp64 sums in a fixed order.
#pragma once
#include "dn_internal.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kErrThreads = 1024;

// f(i) for every i < n with m[i] != 0: the aligned middle of the mask is read four bytes at a time.  The order in which one thread
// meets its pixels is fixed, so the sums are reproducible.
template <typename F>
static __device__ __forceinline__ void for_each_masked(const uint8_t* __restrict__ m, int n, F f) {
  const int tid = threadIdx.x;
  const int head = min(n, (int)((4 - (reinterpret_cast<uintptr_t>(m) & 3)) & 3));
  if (tid < head && m[tid]) f(tid);
  const int nwords = (n - head) / 4;
  const uint32_t* mw = reinterpret_cast<const uint32_t*>(m + head);
  for (int wi = tid; wi < nwords; wi += kErrThreads) {
    const uint32_t v = mw[wi];
    if (v == 0) continue;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if ((v >> (8 * k)) & 255u) f(head + 4 * wi + k);
  }
  const int i = head + 4 * nwords + tid;
  if (i < n && m[i]) f(i);
}

// sum over the block in a fixed tree order; every thread returns the total
template <typename T>
static __device__ __forceinline__ T block_total(T v, T* red) {
  __syncthreads();
  red[threadIdx.x] = v;
  __syncthreads();
  for (int o = kErrThreads / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  return red[0];
}

// The whole of one image (block b).  kClamp: the scaled prediction is clamped to [lo, hi] in fp32 before the metrics (the medians are
// those of the unclamped predictions); without it lo / hi are not read and the arithmetic is dn_eval_errors' as it always was.
template <bool kClamp>
static __device__ __forceinline__ void eval_errors_image(const float* __restrict__ gt, const float* __restrict__ pred,
                                                         const uint8_t* __restrict__ mask, const long long* __restrict__ off,
                                                         const int* __restrict__ npix, int scale_mode, float fixed_scale, float lo, float hi,
                                                         float* __restrict__ out) {
  __shared__ double red[kErrThreads];
  __shared__ unsigned hist[2][256];
  __shared__ unsigned s_prefix[2], s_rank[2], s_more[2], s_next[2];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* g = gt + off[b];
  const float* p = pred + off[b];
  const uint8_t* m = mask + off[b];
  const int n = npix[b];
  float scale = 1.f;
  if (scale_mode == 1) scale = fixed_scale;
  if (scale_mode == 2) {
    // np.median of both arrays: the element of rank (cnt-1)/2 by a 4-pass radix select on the bit patterns (positive values order
    // like their bits), gt in histogram 0 and pred in histogram 1 of the same sweep; for an even count also the next element up
    unsigned prefix[2] = {0, 0}, cnt = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      for (int k = tid; k < 512; k += kErrThreads) hist[k >> 8][k & 255] = 0;
      __syncthreads();
      // a thread's consecutive values mostly share a bucket (all depths share the first byte): count the run, add it once
      unsigned last[2] = {0, 0}, run[2] = {0, 0};
      for_each_masked(m, n, [&](int i) {
        const unsigned bits[2] = {__float_as_uint(g[i]), __float_as_uint(p[i])};
#pragma unroll
        for (int a = 0; a < 2; ++a)
          if (pass == 0 || (bits[a] >> (shift + 8)) == (prefix[a] >> (shift + 8))) {
            const unsigned k = (bits[a] >> shift) & 255u;
            if (k != last[a] && run[a]) {
              atomicAdd(&hist[a][last[a]], run[a]);
              run[a] = 0;
            }
            last[a] = k;
            ++run[a];
          }
      });
#pragma unroll
      for (int a = 0; a < 2; ++a)
        if (run[a]) atomicAdd(&hist[a][last[a]], run[a]);
      __syncthreads();
      if (tid < 2) {
        unsigned r = s_rank[tid];
        if (pass == 0) {
          unsigned c = 0;
          for (int k = 0; k < 256; ++k) c += hist[tid][k];
          r = c > 0 ? (c - 1) / 2 : 0;
          s_next[tid] = c;                      // the count, until the last pass
        }
        unsigned k = 0;
        for (; k < 255; ++k) {
          if (r < hist[tid][k]) break;
          r -= hist[tid][k];
        }
        s_prefix[tid] = prefix[tid] | (k << shift);
        s_rank[tid] = r;
        s_more[tid] = r + 1 < hist[tid][k];     // after the last pass: another copy of the selected value sits above its rank
      }
      __syncthreads();
      prefix[0] = s_prefix[0];
      prefix[1] = s_prefix[1];
      cnt = s_next[0];
      __syncthreads();
    }
    float med[2] = {__uint_as_float(prefix[0]), __uint_as_float(prefix[1])};
    if (cnt > 0 && cnt % 2 == 0) {
      if (tid < 2) s_next[tid] = 0xFFFFFFFFu;
      __syncthreads();
      unsigned mn[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
      for_each_masked(m, n, [&](int i) {
        const unsigned bg = __float_as_uint(g[i]), bp = __float_as_uint(p[i]);
        if (bg > prefix[0]) mn[0] = min(mn[0], bg);
        if (bp > prefix[1]) mn[1] = min(mn[1], bp);
      });
      atomicMin(&s_next[0], mn[0]);
      atomicMin(&s_next[1], mn[1]);
      __syncthreads();
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float up = s_more[a] ? med[a] : __uint_as_float(s_next[a]);
        med[a] = __fdiv_rn(__fadd_rn(med[a], up), 2.f);   // numpy: the fp32 mean of the two middle elements
      }
    }
    scale = cnt > 0 ? __fdiv_rn(med[0], med[1]) : __uint_as_float(0x7FC00000u);
  }
  double s_abs = 0.0, s_sq_rel = 0.0, s_sq = 0.0, s_log = 0.0;
  unsigned c1 = 0, c2 = 0, c3 = 0, cn = 0;
  for_each_masked(m, n, [&](int i) {
    const float gv = g[i];
    float pv = __fmul_rn(p[i], scale);
    if (kClamp) pv = fminf(fmaxf(pv, lo), hi);
    const float thr = fmaxf(__fdiv_rn(gv, pv), __fdiv_rn(pv, gv));
    c1 += thr < 1.25f;
    c2 += thr < 1.5625f;
    c3 += thr < 1.953125f;
    ++cn;
    const double gd = (double)gv, pd = (double)pv;
    const double d = gd - pd, dl = log(gd) - log(pd);
    s_abs += fabs(d) / gd;
    s_sq_rel += d * d / gd;
    s_sq += d * d;
    s_log += dl * dl;
  });
  unsigned* ured = reinterpret_cast<unsigned*>(red);
  const double count = (double)block_total(cn, ured);
  const double r[7] = {block_total(s_abs, red) / count,
                       block_total(s_sq_rel, red) / count,
                       sqrt(block_total(s_sq, red) / count),
                       sqrt(block_total(s_log, red) / count),
                       (double)block_total(c1, ured) / count,
                       (double)block_total(c2, ured) / count,
                       (double)block_total(c3, ured) / count};   // 0 / 0 = NaN for an empty mask, like numpy's mean of nothing
  if (tid < 7) out[b * 8 + tid] = (float)r[tid];
  if (tid == 7) out[b * 8 + 7] = scale;
}

}  // namespace dn
