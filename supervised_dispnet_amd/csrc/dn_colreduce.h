// The two-stage column reduction shared by the HBM-bound NHWC kernels (dn_bn.hip, dn_pointwise.hip, dn_optim.hip): block size and grid
// sizing, the generic column-reduce skeleton with its launcher, and the V-wide channel vector the reduce ops load and store.
// All column reductions are two-stage (per-block partial rows in a caller workspace, then a finalize) so results are
// deterministic and no float atomics are used.  Device code only; not part of the ABI.
#pragma once
#include "dn_device.h"

namespace dn {

constexpr int kThreads = 256;
constexpr int kMaxReduceBlocks = 4096;

static inline int ew_blocks(long long n_items) {
  long long b = (n_items + kThreads - 1) / kThreads;
  if (b > 4096) b = 4096;
  if (b < 1) b = 1;
  return (int)b;
}

static inline int reduce_blocks(long long rows, int C) {
  int V = (C % 4 == 0) ? 4 : 1;
  int groups = C / V;
  int tpr = 1;
  while (tpr < groups && tpr < kThreads) tpr <<= 1;
  int rpi = kThreads / tpr;
  const int rpt = 2;        // rows each thread walks (2: 8 left a 4-image shard 416 blocks of 8 dependent row visits each)
  long long b = (rows + (long long)rpi * rpt - 1) / ((long long)rpi * rpt);
  const int cap = 1024 < kMaxReduceBlocks ? 1024 : kMaxReduceBlocks;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// ---------------------------------------------------------------------------------- generic column-reduce skeleton
// Op::apply<V>(row, c0, acc[V][NACC]) does the element-wise work for channels [c0, c0+V) of `row` and accumulates.
template <class Op, int V>
__global__ void __launch_bounds__(kThreads) colreduce_kernel(Op op, long long rows, int C, float* __restrict__ partial) {
  constexpr int NACC = Op::NACC;
  const int groups = C / V;
  int tpr = 1;
  while (tpr < groups && tpr < kThreads) tpr <<= 1;
  const int rpi = kThreads / tpr;
  const int rl = threadIdx.x / tpr, gi = threadIdx.x % tpr;
  const long long per = (rows + gridDim.x - 1) / gridDim.x;
  const long long rbeg = blockIdx.x * per;
  const long long rend = (rbeg + per < rows) ? rbeg + per : rows;
  __shared__ float red[kThreads * V * NACC];
  for (int g0 = 0; g0 < groups; g0 += tpr) {
    const int grp = g0 + gi;
    float acc[V][NACC];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int a = 0; a < NACC; ++a) acc[v][a] = 0.f;
    if (grp < groups)
      for (long long r = rbeg + rl; r < rend; r += rpi) op.template apply<V>(r, grp * V, acc);
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int a = 0; a < NACC; ++a) red[(threadIdx.x * V + v) * NACC + a] = acc[v][a];
    __syncthreads();
    if (rl == 0 && grp < groups) {
#pragma unroll
      for (int v = 0; v < V; ++v)
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
          float s = 0.f;
          for (int q = 0; q < rpi; ++q) s += red[((q * tpr + gi) * V + v) * NACC + a];
          partial[((long long)blockIdx.x * C + grp * V + v) * NACC + a] = s;
        }
    }
    __syncthreads();
  }
}

template <class Op>
static int launch_colreduce(const Op& op, long long rows, int C, float* partial, hipStream_t s, const char* what) {
  const int blocks = reduce_blocks(rows, C);
  if (C % 4 == 0)
    DN_LAUNCH((colreduce_kernel<Op, 4>), dim3(blocks), dim3(kThreads), 0, s, op, rows, C, partial);
  else
    DN_LAUNCH((colreduce_kernel<Op, 1>), dim3(blocks), dim3(kThreads), 0, s, op, rows, C, partial);
  return check_launch(what);
}

template <int V>
struct Vec {
  float v[V];
};
template <int V>
__device__ __forceinline__ Vec<V> ldv(const float* p) {
  Vec<V> r;
  if constexpr (V == 4) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) r.v[i] = t[i];
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) r.v[i] = p[i];
  }
  return r;
}
template <int V>
__device__ __forceinline__ void stv(float* p, const Vec<V>& r) {
  if constexpr (V == 4) {
    *reinterpret_cast<f32x4*>(p) = f32x4{r.v[0], r.v[1], r.v[2], r.v[3]};
  } else {
#pragma unroll
    for (int i = 0; i < V; ++i) p[i] = r.v[i];
  }
}

}  // namespace dn
