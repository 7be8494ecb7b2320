// monodepth2 self-supervision (reference: layers.py:28-103,139-190 and the per-pixel minimum-reprojection loss composed from them).
//   * pose matrices from (axisangle, translation), BackprojectDepth, Project3D: plain element-wise kernels, one thread per batch
//     element / per pixel, inputs read through their element strides;
//   * the fused loss: per source frame ONE launch that warps the tile + its one-pixel halo into LDS (backproject -> project ->
//     bilinear border sample) and evaluates SSIM + L1 out of LDS, so that no point cloud, grid, warped image or SSIM map reaches HBM;
//     the same kernel without the warp stage gives the identity (automask) terms; one select launch takes the minimum.
// No atomics anywhere: sums are per-block partials added in a fixed order.
#include "dn_reproj_dev.h"

namespace dn {

// ------------------------------------------------------------------------------------------------ (axisangle, translation) -> 4x4
// layers.py:64-103: angle = |v|, axis = v / (angle + 1e-7), Rodrigues
__device__ __forceinline__ void rodrigues(const float* v, float* R /*9*/) {
  const float a = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const float inv = 1.f / (a + 1e-7f);
  const float x = v[0] * inv, y = v[1] * inv, z = v[2] * inv;
  const float ca = cosf(a), sa = sinf(a), C = 1.f - ca;
  const float xs = x * sa, ys = y * sa, zs = z * sa, xC = x * C, yC = y * C, zC = z * C;
  const float xyC = x * yC, yzC = y * zC, zxC = z * xC;
  R[0] = x * xC + ca; R[1] = xyC - zs;    R[2] = zxC + ys;
  R[3] = xyC + zs;    R[4] = y * yC + ca; R[5] = yzC - xs;
  R[6] = zxC - ys;    R[7] = yzC + xs;    R[8] = z * zC + ca;
}

// dL/dv from G = dL/dR
__device__ __forceinline__ void rodrigues_bwd(const float* v, const float* G, float* dv) {
  const float a = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
  const float inv = 1.f / (a + 1e-7f);
  const float x = v[0] * inv, y = v[1] * inv, z = v[2] * inv;
  const float ca = cosf(a), sa = sinf(a), C = 1.f - ca;
  const float s01 = G[1] + G[3], s02 = G[2] + G[6], s12 = G[5] + G[7];
  const float dC = G[0] * x * x + G[4] * y * y + G[8] * z * z + s01 * x * y + s02 * z * x + s12 * y * z;
  const float dca = (G[0] + G[4] + G[8]) - dC;
  const float dsa = z * (G[3] - G[1]) + y * (G[2] - G[6]) + x * (G[7] - G[5]);
  const float dx = 2.f * x * C * G[0] + y * C * s01 + z * C * s02 + sa * (G[7] - G[5]);
  const float dy = 2.f * y * C * G[4] + x * C * s01 + z * C * s12 + sa * (G[2] - G[6]);
  const float dz = 2.f * z * C * G[8] + x * C * s02 + y * C * s12 + sa * (G[3] - G[1]);
  const float dinv = dx * v[0] + dy * v[1] + dz * v[2];
  const float da = -dca * sa + dsa * ca - dinv * inv * inv;
  const float ia = a > 0.f ? 1.f / a : 0.f;                     // torch.norm's subgradient at 0
  dv[0] = dx * inv + da * v[0] * ia;
  dv[1] = dy * inv + da * v[1] * ia;
  dv[2] = dz * inv + da * v[2] * ia;
}

// mode 0: rot_from_axisangle, 1: get_translation_matrix, 2: transformation_from_parameters (M = T R; inverted: M = R^T T(-t))
__device__ __forceinline__ void pose_matrix(const float* v, const float* t, int mode, bool invert, float* M /*16*/) {
  float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
  float tr[3] = {0.f, 0.f, 0.f};
  if (mode != 1) rodrigues(v, R);
  if (mode != 0)
    for (int i = 0; i < 3; ++i) tr[i] = t[i];
  if (mode == 2 && invert) {
    float A[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) A[i * 3 + j] = R[j * 3 + i];
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) M[i * 4 + j] = A[i * 3 + j];
      M[i * 4 + 3] = A[i * 3] * -tr[0] + A[i * 3 + 1] * -tr[1] + A[i * 3 + 2] * -tr[2];
    }
  } else {
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 3; ++j) M[i * 4 + j] = R[i * 3 + j];
      M[i * 4 + 3] = tr[i];
    }
  }
  M[12] = 0.f; M[13] = 0.f; M[14] = 0.f; M[15] = 1.f;
}

__device__ __forceinline__ void pose_matrix_bwd(const float* v, const float* t, int mode, bool invert, const float* dM, float* dv, float* dt) {
  float G[9];
  dv[0] = dv[1] = dv[2] = 0.f;
  dt[0] = dt[1] = dt[2] = 0.f;
  if (mode == 2 && invert) {
    float R[9];
    rodrigues(v, R);
    const float dm[3] = {dM[3], dM[7], dM[11]};
    // A = R^T, m = -A t:  dA[i][j] = dM[i][j] - dm[i] t[j];  dR[j][i] = dA[i][j];  dt = -R dm
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[j * 3 + i] = dM[i * 4 + j] - dm[i] * t[j];
    for (int i = 0; i < 3; ++i) dt[i] = -(R[i * 3] * dm[0] + R[i * 3 + 1] * dm[1] + R[i * 3 + 2] * dm[2]);
    rodrigues_bwd(v, G, dv);
    return;
  }
  if (mode != 1) {
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) G[i * 3 + j] = dM[i * 4 + j];
    rodrigues_bwd(v, G, dv);
  }
  if (mode != 0)
    for (int i = 0; i < 3; ++i) dt[i] = dM[i * 4 + 3];
}

// element (b, f, e) of a strided [B][F][3] view
struct Vec3View {
  const float* p;
  long long sb, sf, se;
};
struct Vec3Out {
  float* p;
  long long sb, sf, se;
};

__device__ __forceinline__ void load3(const Vec3View& a, int b, int f, float* o) {
  if (a.p == nullptr) { o[0] = o[1] = o[2] = 0.f; return; }
  const float* q = a.p + b * a.sb + f * a.sf;
  o[0] = q[0]; o[1] = q[a.se]; o[2] = q[2 * a.se];
}

// one thread per (frame, batch element); M [F][B][16]
__global__ void pose_matrix_fwd_kernel(Vec3View aa, Vec3View tr, int B, int F, int mode, unsigned invert_mask, float* __restrict__ M) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * F) return;
  const int f = i / B, b = i - f * B;
  float v[3], t[3], m[16];
  load3(aa, b, f, v);
  load3(tr, b, f, t);
  pose_matrix(v, t, mode, (invert_mask >> f) & 1u, m);
  for (int k = 0; k < 16; ++k) M[(long long)i * 16 + k] = m[k];
}

__global__ void pose_matrix_bwd_kernel(Vec3View aa, Vec3View tr, int B, int F, int mode, unsigned invert_mask, const float* __restrict__ dM,
                                       Vec3Out daa, Vec3Out dtr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * F) return;
  const int f = i / B, b = i - f * B;
  float v[3], t[3], g[16], dv[3], dt[3];
  load3(aa, b, f, v);
  load3(tr, b, f, t);
  for (int k = 0; k < 16; ++k) g[k] = dM[(long long)i * 16 + k];
  pose_matrix_bwd(v, t, mode, (invert_mask >> f) & 1u, g, dv, dt);
  if (daa.p != nullptr)
    for (int k = 0; k < 3; ++k) daa.p[b * daa.sb + f * daa.sf + k * daa.se] = dv[k];
  if (dtr.p != nullptr)
    for (int k = 0; k < 3; ++k) dtr.p[b * dtr.sb + f * dtr.sf + k * dtr.se] = dt[k];
}

// ------------------------------------------------------------------------------------------------ BackprojectDepth / Project3D

// out [B][4][HW]: rows 0-2 = depth * invK[:3,:3] (x, y, 1), row 3 = 1.  invK [B][16].
__global__ void backproject_fwd_kernel(const float* __restrict__ depth, const float* __restrict__ invK, int B, int H, int W,
                                       float* __restrict__ out) {
  const long long plane = (long long)H * W, total = (long long)B * plane;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / plane);
    const long long p = i - (long long)b * plane;
    const float x = (float)(p % W), y = (float)(p / W);
    const float* k = invK + b * 16;
    const float d = depth[i];
    float* o = out + (long long)b * 4 * plane + p;
    for (int r = 0; r < 3; ++r) o[r * plane] = d * (k[r * 4] * x + k[r * 4 + 1] * y + k[r * 4 + 2]);
    o[3 * plane] = 1.f;
  }
}

__global__ void backproject_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ invK, int B, int H, int W,
                                       float* __restrict__ ddepth) {
  const long long plane = (long long)H * W, total = (long long)B * plane;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int b = (int)(i / plane);
    const long long p = i - (long long)b * plane;
    const float x = (float)(p % W), y = (float)(p / W);
    const float* k = invK + b * 16;
    const float* g = dout + (long long)b * 4 * plane + p;
    float s = 0.f;
    for (int r = 0; r < 3; ++r) s += g[r * plane] * (k[r * 4] * x + k[r * 4 + 1] * y + k[r * 4 + 2]);
    ddepth[i] = s;
  }
}


// grid [B][H][W][2]: pix = c[:2] / (c[2] + eps), x /= W-1, y /= H-1, (. - 0.5) * 2.  No clamp on c[2].  grid (blocks, B).
__global__ void __launch_bounds__(256) project3d_fwd_kernel(const float* __restrict__ pts, const float* __restrict__ K,
                                                            const float* __restrict__ T, int H, int W, float eps, float* __restrict__ grid) {
  const int b = blockIdx.y;
  const long long plane = (long long)H * W;
  __shared__ float P[12];
  if (threadIdx.x == 0) proj_matrix(K, T, b, P);
  __syncthreads();
  const float* q = pts + (long long)b * 4 * plane;
  for (long long p = blockIdx.x * 256ll + threadIdx.x; p < plane; p += (long long)gridDim.x * 256) {
    const float a0 = q[p], a1 = q[plane + p], a2 = q[2 * plane + p], a3 = q[3 * plane + p];
    const float c0 = P[0] * a0 + P[1] * a1 + P[2] * a2 + P[3] * a3;
    const float c1 = P[4] * a0 + P[5] * a1 + P[6] * a2 + P[7] * a3;
    const float z = (P[8] * a0 + P[9] * a1 + P[10] * a2 + P[11] * a3) + eps;
    float* o = grid + ((long long)b * plane + p) * 2;
    o[0] = ((c0 / z) / (float)(W - 1) - 0.5f) * 2.f;
    o[1] = ((c1 / z) / (float)(H - 1) - 0.5f) * 2.f;
  }
}

// dpoints [B][4][HW] and the per-block partial sums of dP [B][gridDim.x][12]
__global__ void __launch_bounds__(256) project3d_bwd_kernel(const float* __restrict__ pts, const float* __restrict__ K,
                                                            const float* __restrict__ T, const float* __restrict__ dgrid, int H, int W,
                                                            float eps, float* __restrict__ dpts, float* __restrict__ partial) {
  const int b = blockIdx.y;
  const long long plane = (long long)H * W;
  __shared__ float P[12];
  __shared__ float lds[48];
  if (threadIdx.x == 0) proj_matrix(K, T, b, P);
  __syncthreads();
  const float* q = pts + (long long)b * 4 * plane;
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  for (long long p = blockIdx.x * 256ll + threadIdx.x; p < plane; p += (long long)gridDim.x * 256) {
    const float a[4] = {q[p], q[plane + p], q[2 * plane + p], q[3 * plane + p]};
    const float c0 = P[0] * a[0] + P[1] * a[1] + P[2] * a[2] + P[3] * a[3];
    const float c1 = P[4] * a[0] + P[5] * a[1] + P[6] * a[2] + P[7] * a[3];
    const float z = (P[8] * a[0] + P[9] * a[1] + P[10] * a[2] + P[11] * a[3]) + eps;
    const float* g = dgrid + ((long long)b * plane + p) * 2;
    const float gpx = g[0] * 2.f / (float)(W - 1), gpy = g[1] * 2.f / (float)(H - 1);
    const float dc[3] = {gpx / z, gpy / z, -(gpx * c0 + gpy * c1) / (z * z)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      dpts[((long long)b * 4 + k) * plane + p] = P[k] * dc[0] + P[4 + k] * dc[1] + P[8 + k] * dc[2];
#pragma unroll
      for (int r = 0; r < 3; ++r) acc[r * 4 + k] += dc[r] * a[k];
    }
  }
  block_sum12(acc, lds, partial + ((long long)b * gridDim.x + blockIdx.x) * 12);
}

// partial [F][B][nblk][12] -> dT [F][B][16] = K[:3,:]^T dP (row 3 of K does not reach P), and / or the gradient of the pose
// parameters the matrices were built from (mode 2).  One thread per (frame, batch element); fixed summation order.
__global__ void reproj_pose_bwd_kernel(const float* __restrict__ partial, int nblk, const float* __restrict__ K, int B, int F,
                                       float* __restrict__ dT, Vec3View aa, Vec3View tr, unsigned invert_mask, Vec3Out daa, Vec3Out dtr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * F) return;
  const int f = i / B, b = i - f * B;
  float dP[12];
  for (int k = 0; k < 12; ++k) dP[k] = 0.f;
  for (int n = 0; n < nblk; ++n)
    for (int k = 0; k < 12; ++k) dP[k] += partial[((long long)i * nblk + n) * 12 + k];
  const float* k4 = K + b * 16;
  float g[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) g[r * 4 + c] = k4[r] * dP[c] + k4[4 + r] * dP[4 + c] + k4[8 + r] * dP[8 + c];
  if (dT != nullptr)
    for (int k = 0; k < 16; ++k) dT[(long long)i * 16 + k] = g[k];
  if (daa.p != nullptr) {
    float v[3], t[3], dv[3], dt[3];
    load3(aa, b, f, v);
    load3(tr, b, f, t);
    pose_matrix_bwd(v, t, 2, (invert_mask >> f) & 1u, g, dv, dt);
    for (int k = 0; k < 3; ++k) {
      daa.p[b * daa.sb + f * daa.sf + k * daa.se] = dv[k];
      dtr.p[b * dtr.sb + f * dtr.sf + k * dtr.se] = dt[k];
    }
  }
}

// ------------------------------------------------------------------------------------------------ the fused loss
// (device code: dn_reproj_dev.h, shared with the multi-scale objective of dn_mono2.hip)

// term[b][y][x] = w * mean_c SSIM(pred, tgt) + (1 - w) * mean_c |tgt - pred|.  grid (tiles x, tiles y, B), 256 threads.
template <bool WARP>
__global__ void __launch_bounds__(256) reproj_term_kernel(const ReprojArgs a, float* __restrict__ term) {
  __shared__ float sx[3][kHN], sy[3][kHN];
  __shared__ float P[12];
  const DispFull disp = {a.disp, a.H, a.W};
  reproj_term_tile<WARP>(a, disp, blockIdx.z, blockIdx.y * kTH, blockIdx.x * kTW, sx, sy, P, term);
}

// m = min over the C channels of terms [C][n] (a tie goes to the lowest channel), sel = its index, partial[block] = sum of m
__global__ void __launch_bounds__(256) reproj_select_kernel(const float* __restrict__ terms, int C, long long n, float* __restrict__ m,
                                                            unsigned char* __restrict__ sel, float* __restrict__ partial) {
  float acc = 0.f;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float best = terms[i];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const float v = terms[(long long)c * n + i];
      if (v < best) { best = v; bi = c; }
    }
    m[i] = best;
    sel[i] = (unsigned char)bi;
    acc += best;
  }
  __shared__ float lds[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// loss = sum(partial) / count: fixed-order fp64 sum by one block (the scheme of sum_finalize_kernel, dn_warp.hip)
__global__ void __launch_bounds__(256) reproj_finalize_kernel(const float* __restrict__ partial, int n, double count, float* __restrict__ loss) {
  __shared__ double lds4[4];
  double s = 0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = (float)(((lds4[0] + lds4[1]) + (lds4[2] + lds4[3])) / count);
}

// upstream gradient of pixel p of sample b for the frame whose reprojection term is channel `channel` of the minimum
struct ReprojUp {
  const unsigned char* sel;   // [B][HW]
  int channel;
  const float* dloss;         // scalar (reduction = mean), scaled by `scale` = 1 / (B H W); or
  const float* dmap;          // [B][HW] (reduction = none)
  float scale;
  __device__ __forceinline__ float operator()(long long i) const {
    if (sel[i] != (unsigned char)channel) return 0.f;
    return dmap != nullptr ? dmap[i] : dloss[0] * scale;
  }
};

// backward pass 1 (reproj_coef_tile): coef [3][B*3][HW].  grid (tiles x, tiles y, B).
__global__ void __launch_bounds__(256) reproj_bwd_coef_kernel(const ReprojArgs a, const ReprojUp u, float* __restrict__ coef) {
  __shared__ float sx[3][kHN], sy[3][kHN];
  __shared__ float P[12];
  const DispFull disp = {a.disp, a.H, a.W};
  reproj_coef_tile(a, disp, u, blockIdx.z, blockIdx.y * kTH, blockIdx.x * kTW, sx, sy, P, coef);
}

// backward pass 2 (reproj_bwd_pixels): ddisp (overwrite / accumulate) and the per-block partial sums of dP [B][gridDim.x][12].
// grid (blocks, B).
__global__ void __launch_bounds__(256) reproj_bwd_kernel(const ReprojArgs a, const ReprojUp u, const float* __restrict__ coef,
                                                         float* __restrict__ ddisp, int accumulate, float* __restrict__ partial) {
  __shared__ float P[12];
  __shared__ float lds[48];
  const int b = blockIdx.y;
  if (threadIdx.x == 0) proj_matrix(a.K, a.T, b, P);
  __syncthreads();
  const DispFull disp = {a.disp, a.H, a.W};
  float acc[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.f;
  reproj_bwd_pixels(a, disp, u, P, b, blockIdx.x * 256ll + threadIdx.x, (long long)gridDim.x * 256, coef, ddisp, accumulate, acc);
  block_sum12(acc, lds, partial + ((long long)b * gridDim.x + blockIdx.x) * 12);
}

static inline dim3 tile_grid(int B, int H, int W) { return dim3((W + kTW - 1) / kTW, (H + kTH - 1) / kTH, B); }

}  // namespace dn

using namespace dn;

extern "C" {

int dn_pose_matrix_fwd(const float* axisangle, int64_t aa_sb, int64_t aa_sf, int64_t aa_se, const float* translation, int64_t t_sb,
                       int64_t t_sf, int64_t t_se, int32_t B, int32_t F, int32_t mode, uint32_t invert_mask, float* M, dn_stream_t stream) {
  DN_REQUIRE(M && B > 0 && F > 0 && F <= 32 && mode >= 0 && mode <= 2 && (mode == 1 || axisangle) && (mode == 0 || translation),
             DN_ERR_BAD_ARG, "dn_pose_matrix_fwd: bad argument");
  const Vec3View aa = {axisangle, aa_sb, aa_sf, aa_se}, tr = {translation, t_sb, t_sf, t_se};
  DN_LAUNCH(pose_matrix_fwd_kernel, dim3((B * F + 63) / 64), dim3(64), 0, as_stream(stream), aa, tr, B, F, mode, invert_mask, M);
  return check_launch("pose_matrix_fwd_kernel");
}

int dn_pose_matrix_bwd(const float* axisangle, int64_t aa_sb, int64_t aa_sf, int64_t aa_se, const float* translation, int64_t t_sb,
                       int64_t t_sf, int64_t t_se, int32_t B, int32_t F, int32_t mode, uint32_t invert_mask, const float* dM,
                       float* daxisangle, float* dtranslation, dn_stream_t stream) {
  DN_REQUIRE(dM && B > 0 && F > 0 && F <= 32 && mode >= 0 && mode <= 2 && (mode == 1 || axisangle) && (mode == 0 || translation),
             DN_ERR_BAD_ARG, "dn_pose_matrix_bwd: bad argument");
  const Vec3View aa = {axisangle, aa_sb, aa_sf, aa_se}, tr = {translation, t_sb, t_sf, t_se};
  const Vec3Out daa = {daxisangle, 3, 3ll * B, 1}, dtr = {dtranslation, 3, 3ll * B, 1};      // contiguous [F][B][3]
  DN_LAUNCH(pose_matrix_bwd_kernel, dim3((B * F + 63) / 64), dim3(64), 0, as_stream(stream), aa, tr, B, F, mode, invert_mask, dM, daa, dtr);
  return check_launch("pose_matrix_bwd_kernel");
}

int dn_backproject_fwd(const float* depth, const float* inv_K, int32_t B, int32_t H, int32_t W, float* points, dn_stream_t stream) {
  DN_REQUIRE(depth && inv_K && points && B > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_backproject_fwd: bad argument");
  DN_LAUNCH(backproject_fwd_kernel, dim3(rp_blocks((long long)B * H * W, 4096)), dim3(256), 0, as_stream(stream), depth, inv_K, B, H, W, points);
  return check_launch("backproject_fwd_kernel");
}

int dn_backproject_bwd(const float* dpoints, const float* inv_K, int32_t B, int32_t H, int32_t W, float* ddepth, dn_stream_t stream) {
  DN_REQUIRE(dpoints && inv_K && ddepth && B > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_backproject_bwd: bad argument");
  DN_LAUNCH(backproject_bwd_kernel, dim3(rp_blocks((long long)B * H * W, 4096)), dim3(256), 0, as_stream(stream), dpoints, inv_K, B, H, W, ddepth);
  return check_launch("backproject_bwd_kernel");
}

int32_t dn_reproj_blocks(int32_t H, int32_t W) { return reproj_blocks(H, W); }

int dn_project3d_fwd(const float* points, const float* K, const float* T, int32_t B, int32_t H, int32_t W, float eps, float* grid,
                     dn_stream_t stream) {
  DN_REQUIRE(points && K && T && grid && B > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_project3d_fwd: bad argument");
  DN_LAUNCH(project3d_fwd_kernel, dim3(reproj_blocks(H, W), B), dim3(256), 0, as_stream(stream), points, K, T, H, W, eps, grid);
  return check_launch("project3d_fwd_kernel");
}

int dn_project3d_bwd(const float* points, const float* K, const float* T, const float* dgrid, int32_t B, int32_t H, int32_t W, float eps,
                     float* dpoints, float* partial, float* dT, dn_stream_t stream) {
  DN_REQUIRE(points && K && T && dgrid && dpoints && partial && dT && B > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "dn_project3d_bwd: bad argument");
  const int nb = reproj_blocks(H, W);
  hipStream_t s = as_stream(stream);
  DN_LAUNCH(project3d_bwd_kernel, dim3(nb, B), dim3(256), 0, s, points, K, T, dgrid, H, W, eps, dpoints, partial);
  const Vec3View none = {nullptr, 0, 0, 0};
  const Vec3Out none_out = {nullptr, 0, 0, 0};
  DN_LAUNCH(reproj_pose_bwd_kernel, dim3((B + 63) / 64), dim3(64), 0, s, (const float*)partial, nb, K, B, 1, dT, none, none, 0u, none_out, none_out);
  return check_launch("project3d_bwd");
}

int dn_reproj_term(const float* tgt, const float* ref, const float* disp, const float* K, const float* inv_K, const float* T, int32_t B,
                   int32_t H, int32_t W, int32_t warp, int32_t align_corners, int32_t disp_mode, float d_lo, float d_span, float eps,
                   float ssim_weight, float* term, dn_stream_t stream) {
  ReprojArgs a;
  int rc = fill_reproj_args(&a, tgt, ref, disp, K, inv_K, T, B, H, W, align_corners, disp_mode, d_lo, d_span, eps, ssim_weight);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(term != nullptr && (!warp || (disp && K && inv_K && T)), DN_ERR_BAD_ARG, "dn_reproj_term: null pointer");
  if (warp) {
    DN_LAUNCH(reproj_term_kernel<true>, tile_grid(B, H, W), dim3(256), 0, as_stream(stream), a, term);
  } else {
    DN_LAUNCH(reproj_term_kernel<false>, tile_grid(B, H, W), dim3(256), 0, as_stream(stream), a, term);
  }
  return check_launch("reproj_term_kernel");
}

int32_t dn_reproj_select_blocks(int64_t n) { return rp_blocks(n, 1024); }

int dn_reproj_select(const float* terms, int32_t C, int64_t n, float* m, uint8_t* sel, float* partial, float* loss, dn_stream_t stream) {
  DN_REQUIRE(terms && m && sel && partial && C >= 1 && C <= 255 && n > 0, DN_ERR_BAD_ARG, "dn_reproj_select: bad argument");
  hipStream_t s = as_stream(stream);
  const int nb = rp_blocks(n, 1024);
  DN_LAUNCH(reproj_select_kernel, dim3(nb), dim3(256), 0, s, terms, C, (long long)n, m, sel, partial);
  if (loss != nullptr) DN_LAUNCH(reproj_finalize_kernel, dim3(1), dim3(256), 0, s, (const float*)partial, nb, (double)n, loss);
  return check_launch("reproj_select");
}

int dn_reproj_bwd(const float* tgt, const float* ref, const float* disp, const float* K, const float* inv_K, const float* T, int32_t B,
                  int32_t H, int32_t W, int32_t align_corners, int32_t disp_mode, float d_lo, float d_span, float eps, float ssim_weight,
                  const uint8_t* sel, int32_t channel, const float* dloss, const float* dmap, float* workspace, float* ddisp,
                  int32_t accumulate, float* partial, dn_stream_t stream) {
  ReprojArgs a;
  int rc = fill_reproj_args(&a, tgt, ref, disp, K, inv_K, T, B, H, W, align_corners, disp_mode, d_lo, d_span, eps, ssim_weight);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(disp && K && inv_K && T && sel && (dloss || dmap) && workspace && ddisp && partial, DN_ERR_BAD_ARG, "dn_reproj_bwd: null pointer");
  const ReprojUp u = {sel, channel, dloss, dmap, 1.f / ((float)B * (float)H * (float)W)};
  hipStream_t s = as_stream(stream);
  DN_LAUNCH(reproj_bwd_coef_kernel, tile_grid(B, H, W), dim3(256), 0, s, a, u, workspace);
  DN_LAUNCH(reproj_bwd_kernel, dim3(reproj_blocks(H, W), B), dim3(256), 0, s, a, u, (const float*)workspace, ddisp, accumulate, partial);
  return check_launch("reproj_bwd");
}

int dn_reproj_pose_bwd(const float* partial, int32_t nblk, const float* K, int32_t B, int32_t F, float* dT, const float* axisangle,
                       int64_t aa_sb, int64_t aa_sf, int64_t aa_se, const float* translation, int64_t t_sb, int64_t t_sf, int64_t t_se,
                       uint32_t invert_mask, float* daxisangle, float* dtranslation, dn_stream_t stream) {
  DN_REQUIRE(partial && K && nblk > 0 && B > 0 && F > 0 && F <= 32 && (dT || daxisangle), DN_ERR_BAD_ARG, "dn_reproj_pose_bwd: bad argument");
  DN_REQUIRE(!daxisangle || (axisangle && translation && dtranslation), DN_ERR_BAD_ARG, "dn_reproj_pose_bwd: pose gradient without the pose");
  const Vec3View aa = {axisangle, aa_sb, aa_sf, aa_se}, tr = {translation, t_sb, t_sf, t_se};
  // the gradients mirror the layout of the parameters they belong to (one [B, F, 6]-like base)
  const Vec3Out daa = {daxisangle, aa_sb, aa_sf, aa_se}, dtr = {dtranslation, t_sb, t_sf, t_se};
  DN_LAUNCH(reproj_pose_bwd_kernel, dim3((B * F + 63) / 64), dim3(64), 0, as_stream(stream), partial, nblk, K, B, F, dT, aa, tr, invert_mask, daa, dtr);
  return check_launch("reproj_pose_bwd_kernel");
}

}  // extern "C"
