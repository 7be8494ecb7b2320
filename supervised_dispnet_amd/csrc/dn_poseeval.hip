// Pose evaluation on the device (eval_pose.py, supervised_dispnet_amd/pose_eval.py): what surrounds the batched
// forward of a pose network between the resized uint8 frames and the two error numbers of a snippet.
//   dn_snippet_gather   snippets (sfmlearner: target first, then the references; monodepth2: the pair) assembled from a ring of resized
//                       uint8 frames into ONE channel-concatenated network input, normalised in IEEE fp32 in dn_eval_normalize's order;
//   dn_pose_eval_sfm    SfMLearner's test_pose.py per snippet: pose vectors -> [R|t] in fp64, inverted and re-based on the first frame,
//                       the least-squares scale against the ground truth, ATE and RE;
//   dn_pose_eval_mono2  monodepth2's evaluate_pose.py per window of track - 1 consecutive pair transforms: both trajectories chained from
//                       the identity, the least-squares scale, ATE.
// The metric kernels run one thread per snippet / window, every sum in index order in fp64 without contraction: no atomics, no
// cross-thread reduction, two runs give the same bits.  They are latency-sized (a few hundred threads of a few hundred flops); what they
// buy is that nothing between the forward and the [N][2] / [P] doubles waits for the host.
#include "dn_internal.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kGatherThreads = 256;
constexpr int kGatherMaxBlocks = 8192;
constexpr int kMetricThreads = 64;

struct Norm3 {
  float m[3], s[3];
};

static __device__ __forceinline__ float norm_u8(unsigned v, float mean, float sd) {
  return __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), mean), sd);
}

// One thread per group of 4 consecutive pixels of one (snippet, frame) plane.  VEC: H * W is a multiple of 4 and both bases are aligned,
// so the 12 bytes of a group are three aligned words and each channel's 4 results one aligned float4; otherwise the group's pixels go
// one by one (the last group of a plane may be short).
template <bool VEC>
__global__ void __launch_bounds__(kGatherThreads) snippet_gather_kernel(const uint8_t* __restrict__ ring, int R, const int* __restrict__ idx,
                                                                        long long groups, int K, long long HW, Norm3 nm,
                                                                        float* __restrict__ dst) {
  const long long gpp = (HW + 3) / 4;                       // groups per plane
  for (long long g = blockIdx.x * (long long)kGatherThreads + threadIdx.x; g < groups; g += (long long)gridDim.x * kGatherThreads) {
    const long long plane = g / gpp;                        // = n * K + k
    const long long p0 = (g - plane * gpp) * 4;
    const long long n = plane / K;
    const int k = (int)(plane - n * K);
    int slot = idx[plane] % R;
    if (slot < 0) slot += R;                                // any table stays inside the ring
    const uint8_t* src = ring + ((long long)slot * HW + p0) * 3;
    float* d0 = dst + ((n * K + k) * 3) * HW + p0;
    if (VEC) {
      const uint32_t* sw = reinterpret_cast<const uint32_t*>(src);
      const uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2];
      // bytes: r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
      float4 r, gch, b;
      r.x = norm_u8(w0 & 255u, nm.m[0], nm.s[0]);
      gch.x = norm_u8((w0 >> 8) & 255u, nm.m[1], nm.s[1]);
      b.x = norm_u8((w0 >> 16) & 255u, nm.m[2], nm.s[2]);
      r.y = norm_u8(w0 >> 24, nm.m[0], nm.s[0]);
      gch.y = norm_u8(w1 & 255u, nm.m[1], nm.s[1]);
      b.y = norm_u8((w1 >> 8) & 255u, nm.m[2], nm.s[2]);
      r.z = norm_u8((w1 >> 16) & 255u, nm.m[0], nm.s[0]);
      gch.z = norm_u8(w1 >> 24, nm.m[1], nm.s[1]);
      b.z = norm_u8(w2 & 255u, nm.m[2], nm.s[2]);
      r.w = norm_u8((w2 >> 8) & 255u, nm.m[0], nm.s[0]);
      gch.w = norm_u8((w2 >> 16) & 255u, nm.m[1], nm.s[1]);
      b.w = norm_u8(w2 >> 24, nm.m[2], nm.s[2]);
      *reinterpret_cast<float4*>(d0) = r;
      *reinterpret_cast<float4*>(d0 + HW) = gch;
      *reinterpret_cast<float4*>(d0 + 2 * HW) = b;
    } else {
      const int cnt = (int)(HW - p0 < 4 ? HW - p0 : 4);
      for (int j = 0; j < cnt; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) d0[c * HW + j] = norm_u8(src[3 * j + c], nm.m[c], nm.s[c]);
    }
  }
}

// ---- 3 x 3 helpers (row-major), fp64
static __device__ __forceinline__ void mat3_mul(const double* a, const double* b, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) o[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

static __device__ __forceinline__ void mat3_vec(const double* a, const double* v, double* o) {
#pragma unroll
  for (int i = 0; i < 3; ++i) o[i] = (a[3 * i] * v[0] + a[3 * i + 1] * v[1]) + a[3 * i + 2] * v[2];
}

// inverse by cofactors: adj(A) / det(A), det expanded along the first row
static __device__ __forceinline__ void mat3_inv(const double* a, double* o) {
  const double c00 = a[4] * a[8] - a[5] * a[7], c01 = a[5] * a[6] - a[3] * a[8], c02 = a[3] * a[7] - a[4] * a[6];
  const double det = (a[0] * c00 + a[1] * c01) + a[2] * c02;
  o[0] = c00 / det;
  o[1] = (a[2] * a[7] - a[1] * a[8]) / det;
  o[2] = (a[1] * a[5] - a[2] * a[4]) / det;
  o[3] = c01 / det;
  o[4] = (a[0] * a[8] - a[2] * a[6]) / det;
  o[5] = (a[2] * a[3] - a[0] * a[5]) / det;
  o[6] = c02 / det;
  o[7] = (a[1] * a[6] - a[0] * a[7]) / det;
  o[8] = (a[0] * a[4] - a[1] * a[3]) / det;
}

// inverse_warp.pose_vec2mat of one (tx, ty, tz, rx, ry, rz), fp64 from the fp32 vector (v == nullptr: the zero vector of the target)
static __device__ void pose_vec2mat64(const float* v, int quat, double* Rm, double* t) {
  double x = 0.0, y = 0.0, z = 0.0;
  t[0] = t[1] = t[2] = 0.0;
  if (v) {
    t[0] = (double)v[0];
    t[1] = (double)v[1];
    t[2] = (double)v[2];
    x = (double)v[3];
    y = (double)v[4];
    z = (double)v[5];
  }
  if (!quat) {                                             // Rx(x) Ry(y) Rz(z)
    const double cx = cos(x), sx = sin(x), cy = cos(y), sy = sin(y), cz = cos(z), sz = sin(z);
    Rm[0] = cy * cz;
    Rm[1] = -(cy * sz);
    Rm[2] = sy;
    Rm[3] = cx * sz + (sx * sy) * cz;
    Rm[4] = cx * cz - (sx * sy) * sz;
    Rm[5] = -(sx * cy);
    Rm[6] = sx * sz - (cx * sy) * cz;
    Rm[7] = sx * cz + (cx * sy) * sz;
    Rm[8] = cx * cy;
  } else {                                                 // (1, x, y, z) normalised
    const double nrm = sqrt(((1.0 + x * x) + y * y) + z * z);
    const double w = 1.0 / nrm;
    x = x / nrm;
    y = y / nrm;
    z = z / nrm;
    const double w2 = w * w, x2 = x * x, y2 = y * y, z2 = z * z;
    const double wx = w * x, wy = w * y, wz = w * z, xy = x * y, xz = x * z, yz = y * z;
    Rm[0] = ((w2 + x2) - y2) - z2;
    Rm[1] = 2.0 * xy - 2.0 * wz;
    Rm[2] = 2.0 * wy + 2.0 * xz;
    Rm[3] = 2.0 * wz + 2.0 * xy;
    Rm[4] = ((w2 - x2) + y2) - z2;
    Rm[5] = 2.0 * yz - 2.0 * wx;
    Rm[6] = 2.0 * xz - 2.0 * wy;
    Rm[7] = 2.0 * wx + 2.0 * yz;
    Rm[8] = ((w2 - x2) - y2) + z2;
  }
}

// frame k of snippet n re-based on frame 0: F_k = [M_0r inv(M_kr) | M_0r (-inv(M_kr) M_kt) + M_0t]
static __device__ void sfm_final_pose(const float* pose, int k, int L, int quat, const double* R0, const double* t0, double* Fr, double* Ft) {
  const int mid = L / 2;
  const float* v = k == mid ? nullptr : pose + 6 * (k < mid ? k : k - 1);
  double Mr[9], Mt[3], Rk[9], tk[3];
  pose_vec2mat64(v, quat, Mr, Mt);
  mat3_inv(Mr, Rk);
  mat3_vec(Rk, Mt, tk);
#pragma unroll
  for (int i = 0; i < 3; ++i) tk[i] = -tk[i];
  mat3_mul(R0, Rk, Fr);
  mat3_vec(R0, tk, Ft);
#pragma unroll
  for (int i = 0; i < 3; ++i) Ft[i] = Ft[i] + t0[i];
}

__global__ void __launch_bounds__(kMetricThreads) pose_eval_sfm_kernel(const float* __restrict__ pose, int quat, const double* __restrict__ gt,
                                                                       int N, int L, double* __restrict__ out) {
  const int n = blockIdx.x * kMetricThreads + threadIdx.x;
  if (n >= N) return;
  const float* pv = pose + (long long)n * (L - 1) * 6;
  const double* g = gt + (long long)n * L * 12;
  double R0[9], t0[3];
  pose_vec2mat64(L / 2 == 0 ? nullptr : pv, quat, R0, t0);   // P_0 (the zero row sits at L / 2 >= 1 for L >= 2)
  double num = 0.0, den = 0.0, re = 0.0;
  for (int k = 0; k < L; ++k) {
    double Fr[9], Ft[3], Fi[9], D[9], G[9];
    sfm_final_pose(pv, k, L, quat, R0, t0, Fr, Ft);
    const double* gk = g + 12 * k;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      num += gk[4 * i + 3] * Ft[i];
      den += Ft[i] * Ft[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) G[3 * i + j] = gk[4 * i + j];
    }
    mat3_inv(Fr, Fi);
    mat3_mul(G, Fi, D);
    const double a = D[1] - D[3], b = D[5] - D[7], c = D[2] - D[6];
    const double s = sqrt((a * a + b * b) + c * c);
    const double cs = ((D[0] + D[4]) + D[8]) - 1.0;
    re += atan2(s, cs);
  }
  const double scale = num / den;                          // 0 / 0 = NaN for all-zero predicted translations, as numpy's
  double ss = 0.0;
  for (int k = 0; k < L; ++k) {
    double Fr[9], Ft[3];
    sfm_final_pose(pv, k, L, quat, R0, t0, Fr, Ft);
    const double* gk = g + 12 * k;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double d = gk[4 * i + 3] - scale * Ft[i];
      ss += d * d;
    }
  }
  out[2 * n] = sqrt(ss) / (double)L;
  out[2 * n + 1] = re / (double)L;
}

// layers.transformation_from_parameters(axisangle, translation, invert=False) = [Rodrigues(axisangle) | translation], fp64 from fp32
static __device__ void mono2_transform64(const float* v, double* Rm, double* t) {
  const double x0 = (double)v[0], y0 = (double)v[1], z0 = (double)v[2];
  t[0] = (double)v[3];
  t[1] = (double)v[4];
  t[2] = (double)v[5];
  const double angle = sqrt((x0 * x0 + y0 * y0) + z0 * z0);
  const double dn = angle + 1e-7;
  const double x = x0 / dn, y = y0 / dn, z = z0 / dn;
  const double ca = cos(angle), sa = sin(angle), C = 1.0 - ca;
  const double xs = x * sa, ys = y * sa, zs = z * sa, xC = x * C, yC = y * C, zC = z * C;
  const double xyC = x * yC, yzC = y * zC, zxC = z * xC;
  Rm[0] = x * xC + ca;
  Rm[1] = xyC - zs;
  Rm[2] = zxC + ys;
  Rm[3] = xyC + zs;
  Rm[4] = y * yC + ca;
  Rm[5] = yzC - xs;
  Rm[6] = zxC - ys;
  Rm[7] = yzC + xs;
  Rm[8] = z * zC + ca;
}

// C <- C T on [R | t] with the implied last row (0, 0, 0, 1)
static __device__ __forceinline__ void affine_chain(double* Cr, double* Ct, const double* Tr, const double* Tt) {
  double nr[9], nt[3];
  mat3_mul(Cr, Tr, nr);
  mat3_vec(Cr, Tt, nt);
#pragma unroll
  for (int i = 0; i < 3; ++i) Ct[i] = nt[i] + Ct[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) Cr[i] = nr[i];
}

static __device__ __forceinline__ void affine_identity(double* Cr, double* Ct) {
#pragma unroll
  for (int i = 0; i < 9; ++i) Cr[i] = (i % 4 == 0) ? 1.0 : 0.0;
  Ct[0] = Ct[1] = Ct[2] = 0.0;
}

static __device__ __forceinline__ void affine_from44(const double* q, double* Tr, double* Tt) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) Tr[3 * i + j] = q[4 * i + j];
    Tt[i] = q[4 * i + 3];
  }
}

__global__ void __launch_bounds__(kMetricThreads) pose_eval_mono2_kernel(const float* __restrict__ pose, const double* __restrict__ Q, int P,
                                                                         int track, double* __restrict__ out) {
  const int i = blockIdx.x * kMetricThreads + threadIdx.x;
  if (i >= P) return;
  const int last = i + track - 1 < P ? i + track - 1 : P;  // transforms i .. last - 1, points 0 .. last - i
  const int nt = last - i;
  double scale = 0.0, ss = 0.0;
  // pass 0: the sums of the scale; pass 1: the residual.  Point 0 of both trajectories is the origin, so the offset gt_0 - pred_0 the
  // original adds is exactly zero and point 0 contributes exact zeros to every sum.
  for (int pass = 0; pass < 2; ++pass) {
    double Cr[9], Ct[3], Gr[9], Gt[3];
    affine_identity(Cr, Ct);
    affine_identity(Gr, Gt);
    double num = 0.0, den = 0.0;
    for (int j = 0; j < nt; ++j) {
      double Tr[9], Tt[3];
      mono2_transform64(pose + 6LL * (i + j), Tr, Tt);
      affine_chain(Cr, Ct, Tr, Tt);
      affine_from44(Q + 16LL * (i + j), Tr, Tt);
      affine_chain(Gr, Gt, Tr, Tt);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (pass == 0) {
          num += Gt[c] * Ct[c];
          den += Ct[c] * Ct[c];
        } else {
          const double d = scale * Ct[c] - Gt[c];
          ss += d * d;
        }
      }
    }
    if (pass == 0) scale = num / den;
  }
  out[i] = sqrt(ss) / (double)(nt + 1);
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_snippet_gather(const uint8_t* ring, int32_t R, const int32_t* idx, int32_t N, int32_t K, int32_t H, int32_t W, const float* mean_host,
                      const float* std_host, float* dst, dn_stream_t stream) {
  DN_REQUIRE(ring && idx && dst && mean_host && std_host, DN_ERR_BAD_ARG, "dn_snippet_gather: null argument");
  DN_REQUIRE(R > 0 && N > 0 && K > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_snippet_gather: bad shape R=%d N=%d K=%d H=%d W=%d", (int)R, (int)N,
             (int)K, (int)H, (int)W);
  const long long HW = (long long)H * W;
  DN_REQUIRE((long long)N * K <= (1LL << 31) - 1 && HW * 3 * R < (1LL << 40) && (long long)N * K * 3 * HW < (1LL << 40), DN_ERR_UNSUPPORTED,
             "dn_snippet_gather: too large");
  const long long groups = (long long)N * K * ((HW + 3) / 4);
  long long blocks = (groups + kGatherThreads - 1) / kGatherThreads;
  if (blocks > kGatherMaxBlocks) blocks = kGatherMaxBlocks;
  Norm3 nm;
  for (int c = 0; c < 3; ++c) {
    nm.m[c] = mean_host[c];
    nm.s[c] = std_host[c];
  }
  const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(ring) & 3) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0;
  if (vec) {
    DN_LAUNCH(snippet_gather_kernel<true>, dim3((unsigned)blocks), dim3(kGatherThreads), 0, as_stream(stream), ring, (int)R, (const int*)idx,
              groups, (int)K, HW, nm, dst);
  } else {
    DN_LAUNCH(snippet_gather_kernel<false>, dim3((unsigned)blocks), dim3(kGatherThreads), 0, as_stream(stream), ring, (int)R, (const int*)idx,
              groups, (int)K, HW, nm, dst);
  }
  return check_launch("snippet_gather_kernel");
}

int dn_pose_eval_sfm(const float* pose, int32_t rotation_mode, const double* gt, int32_t N, int32_t L, double* out, dn_stream_t stream) {
  DN_REQUIRE(pose && gt && out, DN_ERR_BAD_ARG, "dn_pose_eval_sfm: null argument");
  DN_REQUIRE(rotation_mode == 0 || rotation_mode == 1, DN_ERR_BAD_ARG, "dn_pose_eval_sfm: rotation_mode %d (0: euler, 1: quat)", (int)rotation_mode);
  DN_REQUIRE(N > 0 && L >= 2 && L <= DN_POSE_EVAL_MAX_L, DN_ERR_BAD_ARG, "dn_pose_eval_sfm: bad shape N=%d L=%d (2 <= L <= %d)", (int)N, (int)L,
             DN_POSE_EVAL_MAX_L);
  DN_LAUNCH(pose_eval_sfm_kernel, dim3((unsigned)((N + kMetricThreads - 1) / kMetricThreads)), dim3(kMetricThreads), 0, as_stream(stream), pose,
            (int)rotation_mode, gt, (int)N, (int)L, out);
  return check_launch("pose_eval_sfm_kernel");
}

int dn_pose_eval_mono2(const float* pose, const double* Q, int32_t P, int32_t track, double* out, dn_stream_t stream) {
  DN_REQUIRE(pose && Q && out, DN_ERR_BAD_ARG, "dn_pose_eval_mono2: null argument");
  DN_REQUIRE(P > 0 && track >= 2 && track <= DN_POSE_EVAL_MAX_TRACK, DN_ERR_BAD_ARG, "dn_pose_eval_mono2: bad shape P=%d track=%d (2 <= track <= %d)",
             (int)P, (int)track, DN_POSE_EVAL_MAX_TRACK);
  DN_LAUNCH(pose_eval_mono2_kernel, dim3((unsigned)((P + kMetricThreads - 1) / kMetricThreads)), dim3(kMetricThreads), 0, as_stream(stream), pose, Q,
            (int)P, (int)track, out);
  return check_launch("pose_eval_mono2_kernel");
}

}  // extern "C"
