// Tail of monodepth2's PoseDecoder (networks.PoseResnet): after pose_1 the reference computes
//   0.01 * mean_hw(conv1x1(x) + b)          (reference networks/pose_decoder.py:46-52)
// The 1x1 convolution commutes with the spatial mean, so the tail is a spatial reduction followed by a [P, C] x [C, O] product -- on maps
// of 4 x 13 or 6 x 20 pixels.  Composed from the conv and mean blocks it is two launches forward and four backward; here it is one each:
//   dn_pose_tail_fwd   one block per pair: mean[p][c] = (1 / HW) sum_s x[p][s][c] (kept for the backward), then one wave per output,
//                      out[p][o] = scale * (bias[o] + sum_c w[o][c] * mean[p][c]) for o < O_used.  Only the rows the trainer reads are
//                      produced: the result is dense [P][O_used].
//   dn_pose_tail_bwd   one launch, two block roles.  Blocks [0, P * nsplit): dx[p][s][c] = (scale / HW) sum_{o < O_used} dout[p][o] w[o][c],
//                      the row sum formed once per thread and stored over the block's pixels.  The blocks after them: one thread per
//                      element of dw / dbias, dw[o][c] = scale * sum_p dout[p][o] mean[p][c], dbias[o] = scale * sum_p dout[p][o], the
//                      sums over p in index order; rows o >= O_used are written as zeros.
// Every sum has a fixed order and no float atomic is used: two runs are bit-identical.  Plain fp32 FMAs; x and dx are read and written as
// float4 (C % 64 == 0), the parameters and their gradients with scalar accesses (an optimizer arena may place them at any 4-byte offset).
#include "dn_internal.h"

namespace dn {

constexpr int kTailThreads = 256;
constexpr int kTailMaxC = 512;
constexpr int kTailMaxO = 24;
constexpr int kTailSplit = 8;      // most pixel chunks per pair of the backward's dx blocks

typedef float tail_f4 __attribute__((ext_vector_type(4)));

// threads of a block as (pixel group, float4 channel lane): cv = C / 4 lanes per pixel, kTailThreads / cv pixel groups (the threads past
// groups * cv idle when cv does not divide the block)
__global__ void __launch_bounds__(kTailThreads) pose_tail_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                     const float* __restrict__ bias, long long HW, int C, int O_used,
                                                                     float scale, float* __restrict__ mean, float* __restrict__ out) {
  __shared__ float red[kTailThreads * 4];
  __shared__ float smean[kTailMaxC];
  const int p = blockIdx.x;
  const int cv = C >> 2;
  const int groups = kTailThreads / cv;
  const int lane = threadIdx.x % cv, g = threadIdx.x / cv;
  if (g < groups) {
    const tail_f4* X = reinterpret_cast<const tail_f4*>(x + (long long)p * HW * C) + lane;
    tail_f4 s = {0.f, 0.f, 0.f, 0.f};
    for (long long q = g; q < HW; q += groups) s += X[q * cv];
    float* r = red + (g * cv + lane) * 4;
    r[0] = s.x, r[1] = s.y, r[2] = s.z, r[3] = s.w;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += kTailThreads) {
    float t = 0.f;
    for (int q = 0; q < groups; ++q) t += red[q * C + c];
    t = t / (float)HW;
    smean[c] = t;
    mean[(long long)p * C + c] = t;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, wl = threadIdx.x & 63;
  for (int o = wave; o < O_used; o += kTailThreads / 64) {
    const float* W = w + (long long)o * C;
    float t = 0.f;
    for (int c = wl; c < C; c += 64) t = fmaf(W[c], smean[c], t);
    for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
    if (wl == 0) out[(long long)p * O_used + o] = scale * (bias[o] + t);
  }
}

__global__ void __launch_bounds__(kTailThreads) pose_tail_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ mean,
                                                                     const float* __restrict__ w, int P, long long HW, int C, int O,
                                                                     int O_used, float scale, int nsplit, float* __restrict__ dx,
                                                                     float* __restrict__ dw, float* __restrict__ dbias) {
  const int ndx = P * nsplit;
  if ((int)blockIdx.x < ndx) {
    const int p = blockIdx.x / nsplit, part = blockIdx.x % nsplit;
    const int cv = C >> 2;
    const int groups = kTailThreads / cv;
    const int lane = threadIdx.x % cv, g = threadIdx.x / cv;
    if (g >= groups) return;
    const long long per = (HW + nsplit - 1) / nsplit;
    const long long s0 = part * per, s1 = (s0 + per < HW) ? s0 + per : HW;
    const float* D = dout + (long long)p * O_used;
    tail_f4 a = {0.f, 0.f, 0.f, 0.f};
    for (int o = 0; o < O_used; ++o) {
      const float d = D[o];
      const float* W = w + (long long)o * C + lane * 4;
      a.x = fmaf(d, W[0], a.x), a.y = fmaf(d, W[1], a.y), a.z = fmaf(d, W[2], a.z), a.w = fmaf(d, W[3], a.w);
    }
    const float k = scale / (float)HW;
    a *= k;
    tail_f4* DX = reinterpret_cast<tail_f4*>(dx + (long long)p * HW * C) + lane;
    for (long long q = s0 + g; q < s1; q += groups) DX[q * cv] = a;
    return;
  }
  const int i = ((int)blockIdx.x - ndx) * kTailThreads + threadIdx.x;
  const int nw = O * C;
  if (i < nw) {
    const int o = i / C, c = i - o * C;
    float t = 0.f;
    if (o < O_used) {
      for (int p = 0; p < P; ++p) t = fmaf(dout[(long long)p * O_used + o], mean[(long long)p * C + c], t);
      t *= scale;
    }
    dw[i] = t;
  } else if (i < nw + O) {
    const int o = i - nw;
    float t = 0.f;
    if (o < O_used) {
      for (int p = 0; p < P; ++p) t += dout[(long long)p * O_used + o];
      t *= scale;
    }
    dbias[o] = t;
  }
}

static int pose_tail_check(const char* who, int32_t P, int64_t HW, int32_t C, int32_t O, int32_t O_used) {
  DN_REQUIRE(P >= 1 && HW >= 1, DN_ERR_BAD_ARG, "%s: P = %d, HW = %lld (each needs >= 1)", who, (int)P, (long long)HW);
  DN_REQUIRE(C >= 64 && C % 64 == 0 && C <= kTailMaxC, DN_ERR_BAD_ARG, "%s: C = %d (a multiple of 64, at most %d)", who, (int)C, kTailMaxC);
  DN_REQUIRE(1 <= O_used && O_used <= O && O <= kTailMaxO, DN_ERR_BAD_ARG, "%s: O_used = %d, O = %d (1 <= O_used <= O <= %d)", who,
             (int)O_used, (int)O, kTailMaxO);
  DN_REQUIRE((long long)P * HW * C < (1ll << 40) && (long long)P * kTailSplit + 64 < (1ll << 31), DN_ERR_BAD_ARG, "%s: problem too large", who);
  return DN_OK;
}

static inline bool tail_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace dn

using namespace dn;

extern "C" {

int dn_pose_tail_fwd(const float* x, const float* w, const float* bias, int32_t P, int64_t HW, int32_t C, int32_t O, int32_t O_used,
                     float scale, float* mean, float* out, dn_stream_t stream) {
  const int rc = pose_tail_check("dn_pose_tail_fwd", P, HW, C, O, O_used);
  if (rc) return rc;
  DN_REQUIRE(x && w && bias && mean && out && tail_aligned(x), DN_ERR_BAD_ARG, "dn_pose_tail_fwd: null pointer, or x not 16-byte aligned");
  DN_LAUNCH(pose_tail_fwd_kernel, dim3((unsigned)P), dim3(kTailThreads), 0, as_stream(stream), x, w, bias, (long long)HW, (int)C, (int)O_used,
            scale, mean, out);
  set_last_kernel("dn::pose_tail_fwd_kernel");
  return check_launch("pose_tail_fwd_kernel");
}

int dn_pose_tail_bwd(const float* dout, const float* mean, const float* w, int32_t P, int64_t HW, int32_t C, int32_t O, int32_t O_used,
                     float scale, float* dx, float* dw, float* dbias, dn_stream_t stream) {
  const int rc = pose_tail_check("dn_pose_tail_bwd", P, HW, C, O, O_used);
  if (rc) return rc;
  DN_REQUIRE(dout && mean && w && dx && dw && dbias && tail_aligned(dx), DN_ERR_BAD_ARG,
             "dn_pose_tail_bwd: null pointer, or dx not 16-byte aligned");
  const int nsplit = HW < kTailSplit ? (int)HW : kTailSplit;
  const int nparam = (O * C + O + kTailThreads - 1) / kTailThreads;
  DN_LAUNCH(pose_tail_bwd_kernel, dim3((unsigned)(P * nsplit + nparam)), dim3(kTailThreads), 0, as_stream(stream), dout, mean, w, (int)P,
            (long long)HW, (int)C, (int)O, (int)O_used, scale, nsplit, dx, dw, dbias);
  set_last_kernel("dn::pose_tail_bwd_kernel");
  return check_launch("pose_tail_bwd_kernel");
}

}  // extern "C"
