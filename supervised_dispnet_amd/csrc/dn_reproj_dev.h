// Device code of the fused minimum-reprojection loss, shared by csrc/dn_reproj.hip (one disparity map at the image's resolution) and
// csrc/dn_mono2.hip (the decoder's scales, each read through the bilinear upsampling): the tile fill (backproject -> project ->
// bilinear border sample into LDS), the SSIM statistics of a tile, and the bodies of the term, coefficient and gather kernels.  What
// differs between the two is where a pixel's disparity comes from (`Disp`) and what upstream gradient it carries (`Up`).
// Device code only; not part of the ABI.
#pragma once
#include "dn_device.h"

namespace dn {

// P = (K T)[:3, :]  (12 floats) of batch element b
__device__ __forceinline__ void proj_matrix(const float* K, const float* T, int b, float* P) {
  const float* k = K + b * 16;
  const float* t = T + b * 16;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) P[r * 4 + c] = k[r * 4] * t[c] + k[r * 4 + 1] * t[4 + c] + k[r * 4 + 2] * t[8 + c] + k[r * 4 + 3] * t[12 + c];
}

// block-wide sum of 12 per-thread values into out[0..12) by thread 0 (256-thread blocks)
__device__ __forceinline__ void block_sum12(float (&v)[12], float* lds /*48*/, float* out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 12; ++i) v[i] = wave_sum(v[i]);
  __syncthreads();
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < 12; ++i) lds[i * 4 + wave] = v[i];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int i = 0; i < 12; ++i) out[i] = (lds[i * 4] + lds[i * 4 + 1]) + (lds[i * 4 + 2] + lds[i * 4 + 3]);
}

struct ReprojArgs {
  const float* tgt;     // [B][3][H][W]
  const float* ref;     // [B][3][H][W] source frame
  const float* disp;    // [B][H][W]
  const float* K;       // [B][16]
  const float* invK;    // [B][16]
  const float* T;       // [B][16] of this frame
  int B, H, W;
  int align;            // grid_sample align_corners
  int disp_mode;        // 1: depth = 1 / (d_lo + d_span * disp) (layers.disp_to_depth); 0: `disp` is the depth
  float d_lo, d_span;   // 1 / max_depth, 1 / min_depth - 1 / max_depth
  float eps;            // Project3D's
  float w;              // ssim_weight
};

// Source of output index o of a bilinear upsampling by the integer factor `scale` (align_corners=False): the half-pixel source index
// clamped at 0, its two neighbours (the upper one clamped at the edge) and the weight of the upper one.  The same definition as
// dn_loss.hip's, which upsample_int_fwd/_bwd_kernel use (that file does not include this header).
__device__ __forceinline__ void bil_src(int o, int scale, int n_in, int* i0, int* i1, float* l1) {
  float s = ((float)o + 0.5f) / (float)scale - 0.5f;
  if (s < 0.f) s = 0.f;
  const int a = (int)s;
  *i0 = a;
  *i1 = a + (a < n_in - 1 ? 1 : 0);
  *l1 = s - (float)a;
}

// the disparity of pixel (y, x) of sample b: the map itself ...
struct DispFull {
  const float* p;
  int H, W;
  __device__ __forceinline__ float operator()(int b, int y, int x) const { return p[((long long)b * H + y) * W + x]; }
};

// ... or a coarse map [B][h][w] upsampled by the integer factor `scale` (bilinear, align_corners=False: bil_src)
struct DispCoarse {
  const float* p;
  int h, w, scale;
  __device__ __forceinline__ float operator()(int b, int y, int x) const {
    const float* L = p + (long long)b * h * w;
    if (scale == 1) return L[y * w + x];
    int y0, y1, x0, x1;
    float ly, lx;
    bil_src(y, scale, h, &y0, &y1, &ly);
    bil_src(x, scale, w, &x0, &x1, &lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    return hy * (hx * L[y0 * w + x0] + lx * L[y0 * w + x1]) + ly * (hx * L[y1 * w + x0] + lx * L[y1 * w + x1]);
  }
};

constexpr int kTW = 32, kTH = 8;                    // output tile of a block: 32 x 8 pixels, one per thread
constexpr int kHW = kTW + 2, kHH = kTH + 2;         // with the one-pixel halo SSIM's 3x3 window needs
constexpr int kHN = kHW * kHH;                      // 340 positions; x 6 planes x 4 B = 8160 B of LDS per block

__device__ __forceinline__ int reflect1r(int v, int n) { return v < 0 ? -v : (v >= n ? 2 * n - 2 - v : v); }

struct ReprojPix {
  float ray[3];          // invK[:3,:3] (x, y, 1)
  float depth;
  float c0, c1, z;       // P [depth * ray; 1], z with eps added
  float ix, iy;          // sample position in pixels, after the border clip
  float mx, my;          // d ix / d xn (0 where clipped)
  int x0, y0;
  bool sane;
};

template <class Disp>
__device__ __forceinline__ void reproj_coords(const ReprojArgs& a, const Disp& disp, const float* P, int b, int y, int x, ReprojPix* q) {
  const float* k = a.invK + b * 16;
  const float fx = (float)x, fy = (float)y;
#pragma unroll
  for (int r = 0; r < 3; ++r) q->ray[r] = k[r * 4] * fx + k[r * 4 + 1] * fy + k[r * 4 + 2];
  const float d = disp(b, y, x);
  q->depth = a.disp_mode ? 1.f / (a.d_lo + a.d_span * d) : d;
  const float p0 = q->depth * q->ray[0], p1 = q->depth * q->ray[1], p2 = q->depth * q->ray[2];
  q->c0 = P[0] * p0 + P[1] * p1 + P[2] * p2 + P[3];
  q->c1 = P[4] * p0 + P[5] * p1 + P[6] * p2 + P[7];
  q->z = (P[8] * p0 + P[9] * p1 + P[10] * p2 + P[11]) + a.eps;
  const float xn = ((q->c0 / q->z) / (float)(a.W - 1) - 0.5f) * 2.f;
  const float yn = ((q->c1 / q->z) / (float)(a.H - 1) - 0.5f) * 2.f;
  float ix, iy, mx, my;
  if (a.align) {
    ix = ((xn + 1.f) / 2.f) * (float)(a.W - 1);
    iy = ((yn + 1.f) / 2.f) * (float)(a.H - 1);
    mx = (float)(a.W - 1) / 2.f;
    my = (float)(a.H - 1) / 2.f;
  } else {
    ix = ((xn + 1.f) * (float)a.W - 1.f) / 2.f;
    iy = ((yn + 1.f) * (float)a.H - 1.f) / 2.f;
    mx = (float)a.W / 2.f;
    my = (float)a.H / 2.f;
  }
  // padding_mode="border": clip_coordinates_set_grad
  if (ix <= 0.f) { ix = 0.f; mx = 0.f; } else if (ix >= (float)(a.W - 1)) { ix = (float)(a.W - 1); mx = 0.f; }
  if (iy <= 0.f) { iy = 0.f; my = 0.f; } else if (iy >= (float)(a.H - 1)) { iy = (float)(a.H - 1); my = 0.f; }
  q->ix = ix; q->iy = iy; q->mx = mx; q->my = my;
  q->sane = ix >= 0.f && ix <= (float)(a.W - 1) && iy >= 0.f && iy <= (float)(a.H - 1);      // false for a NaN coordinate: no tap is read
  q->x0 = q->sane ? (int)floorf(ix) : -10;
  q->y0 = q->sane ? (int)floorf(iy) : -10;
}

// the four taps (nw, ne, sw, se; 0 outside the image) and the bilinear value of the three planes
__device__ __forceinline__ void reproj_sample(const ReprojArgs& a, int b, const ReprojPix& q, float (&tap)[4][3], float (&v)[3]) {
  const float fx0 = floorf(q.ix), fy0 = floorf(q.iy);
  const float wx1 = q.ix - fx0, wx0 = (fx0 + 1.f) - q.ix, wy1 = q.iy - fy0, wy0 = (fy0 + 1.f) - q.iy;
  const long long plane = (long long)a.H * a.W;
  const float* I = a.ref + (long long)b * 3 * plane;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int xx = q.x0 + (t & 1), yy = q.y0 + (t >> 1);
    const bool in = q.sane && xx >= 0 && xx < a.W && yy >= 0 && yy < a.H;
#pragma unroll
    for (int c = 0; c < 3; ++c) tap[t][c] = in ? I[c * plane + (long long)yy * a.W + xx] : 0.f;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = tap[0][c] * (wx0 * wy0) + tap[1][c] * (wx1 * wy0) + tap[2][c] * (wx0 * wy1) + tap[3][c] * (wx1 * wy1);
}

// Fill the tile + halo of the prediction (warped source frame, or the source frame itself) and of the target into LDS.  A halo
// position outside the image holds the value of its reflection (ReflectionPad2d(1)); positions no window of the tile reads hold 0.
template <bool WARP, class Disp>
__device__ __forceinline__ void reproj_fill_tile(const ReprojArgs& a, const Disp& disp, const float* P, int b, int ty0, int tx0,
                                                 float (*sx)[kHN], float (*sy)[kHN]) {
  const long long plane = (long long)a.H * a.W;
  for (int idx = threadIdx.x; idx < kHN; idx += 256) {
    const int hy = idx / kHW, hx = idx - hy * kHW;
    const int gy = ty0 + hy - 1, gx = tx0 + hx - 1;
    float pv[3] = {0.f, 0.f, 0.f}, tv[3] = {0.f, 0.f, 0.f};
    if (gy >= -1 && gy <= a.H && gx >= -1 && gx <= a.W) {
      const int yy = reflect1r(gy, a.H), xx = reflect1r(gx, a.W);
      const long long o = (long long)b * 3 * plane + (long long)yy * a.W + xx;
#pragma unroll
      for (int c = 0; c < 3; ++c) tv[c] = a.tgt[o + c * plane];
      if (WARP) {
        ReprojPix q;
        float tap[4][3];
        reproj_coords(a, disp, P, b, yy, xx, &q);
        reproj_sample(a, b, q, tap, pv);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) pv[c] = a.ref[o + c * plane];
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { sx[c][idx] = pv[c]; sy[c][idx] = tv[c]; }
  }
}

struct SsimStats {
  float mx, my, sx, sy, sxy, n, d;
};

// SSIM statistics of the 3x3 window centred at tile pixel (ly, lx), read from the LDS tile (x = prediction, y = target)
__device__ __forceinline__ SsimStats ssim_tile_stats(const float* X, const float* Y, int ly, int lx) {
  // No FMA contraction (as ssim_stats of dn_warp.hip): SSIM(x, x) must be exactly 1, i.e. n == d bit for bit when Y == X.
  // The (co)variances are sums of centred products, not E[xy] - mu_x mu_y: the window is in LDS, a second pass over it is free, and
  // the subtraction of two numbers of the size of the squared intensity costs fp32 some 1e-5 of the term per pixel (values around
  // 0.5, variances around 1e-3) -- which is what the fp32 restatement on the CPU loses against fp64.
#pragma clang fp contract(off)
  float sx = 0.f, sy = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      sx += X[(ly + dy) * kHW + lx + dx];
      sy += Y[(ly + dy) * kHW + lx + dx];
    }
  SsimStats r;
  r.mx = sx / 9.f;
  r.my = sy / 9.f;
  float vx = 0.f, vy = 0.f, vxy = 0.f;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float a = X[(ly + dy) * kHW + lx + dx] - r.mx, b = Y[(ly + dy) * kHW + lx + dx] - r.my;
      vx += a * a; vy += b * b; vxy += a * b;
    }
  r.sx = vx / 9.f;
  r.sy = vy / 9.f;
  r.sxy = vxy / 9.f;
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
  r.n = (2.f * r.mx * r.my + C1) * (2.f * r.sxy + C2);
  r.d = (r.mx * r.mx + r.my * r.my + C1) * (r.sx + r.sy + C2);
  return r;
}

// One 8 x 32 tile of term[b] = w * mean_c SSIM(pred, tgt) + (1 - w) * mean_c |tgt - pred|; `term` is the [B][H][W] map.
// 256 threads; sx, sy [3][kHN] and P [12] are the block's LDS.
template <bool WARP, class Disp>
__device__ __forceinline__ void reproj_term_tile(const ReprojArgs& a, const Disp& disp, int b, int ty0, int tx0, float (*sx)[kHN],
                                                 float (*sy)[kHN], float* P, float* __restrict__ term) {
  if (WARP) {
    if (threadIdx.x == 0) proj_matrix(a.K, a.T, b, P);
    __syncthreads();
  }
  reproj_fill_tile<WARP>(a, disp, P, b, ty0, tx0, sx, sy);
  __syncthreads();
  const int ly = threadIdx.x / kTW, lx = threadIdx.x % kTW;
  const int y = ty0 + ly, x = tx0 + lx;
  if (y >= a.H || x >= a.W) return;
  float ss = 0.f, l1 = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const SsimStats s = ssim_tile_stats(sx[c], sy[c], ly, lx);
    ss += fminf(fmaxf((1.f - s.n / s.d) / 2.f, 0.f), 1.f);
    l1 += fabsf(sy[c][(ly + 1) * kHW + lx + 1] - sx[c][(ly + 1) * kHW + lx + 1]);
  }
  term[((long long)b * a.H + y) * a.W + x] = a.w * (ss / 3.f) + (1.f - a.w) * (l1 / 3.f);
}

// backward pass 1 on one tile: per window centre and colour plane the three coefficients  g * d ssim / d (mu_x, E[xx], E[xy])  (x = the
// warped frame); coef [3][B*3][HW].  The clamp passes gradient on [0, 1] inclusive, as ssim_bwd_coef_kernel does.  up(i): the upstream
// gradient of pixel i of [B][HW].
template <class Disp, class Up>
__device__ __forceinline__ void reproj_coef_tile(const ReprojArgs& a, const Disp& disp, const Up& up, int b, int ty0, int tx0,
                                                 float (*sx)[kHN], float (*sy)[kHN], float* P, float* __restrict__ coef) {
  if (threadIdx.x == 0) proj_matrix(a.K, a.T, b, P);
  __syncthreads();
  reproj_fill_tile<true>(a, disp, P, b, ty0, tx0, sx, sy);
  __syncthreads();
  const int ly = threadIdx.x / kTW, lx = threadIdx.x % kTW;
  const int y = ty0 + ly, x = tx0 + lx;
  if (y >= a.H || x >= a.W) return;
  const long long plane = (long long)a.H * a.W, total = (long long)a.B * 3 * plane;
  const long long p = (long long)y * a.W + x;
  const float g = up((long long)b * plane + p) * (a.w / 3.f);
  const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const SsimStats s = ssim_tile_stats(sx[c], sy[c], ly, lx);
    const float raw = (1.f - s.n / s.d) / 2.f;
    const float gu = (raw >= 0.f && raw <= 1.f) ? g : 0.f;
    const float dn = -0.5f / s.d * gu, dd = 0.5f * s.n / (s.d * s.d) * gu;
    const float A1 = 2.f * s.mx * s.my + C1, A2 = 2.f * s.sxy + C2, B1 = s.mx * s.mx + s.my * s.my + C1, B2 = s.sx + s.sy + C2;
    const float dA1 = dn * A2, dA2 = dn * A1, dB1 = dd * B2, dB2 = dd * B1;
    const float dsxy = 2.f * dA2, dsx = dB2;
    const float dmx = dA1 * 2.f * s.my + dB1 * 2.f * s.mx - dsxy * s.my - dsx * 2.f * s.mx;
    const long long o = ((long long)b * 3 + c) * plane + p;
    coef[o] = dmx;
    coef[total + o] = dsx;
    coef[2 * total + o] = dsxy;
  }
}

// backward pass 2 for the pixels p = first, first + stride, ... of sample b: every pixel gathers the SSIM gradient of its warped value
// from the window centres that cover it, adds the L1 term, and takes it through the sampler (border clip zeroes the coordinate
// gradient), the projection and the backprojection: ddisp [B][HW] (the gradient of the value `disp` returns; overwrite / accumulate)
// and the sums of dP in acc.  P [12]: the block's projection matrix.
template <class Disp, class Up>
__device__ __forceinline__ void reproj_bwd_pixels(const ReprojArgs& a, const Disp& disp, const Up& up, const float* P, int b, long long first,
                                                  long long stride, const float* __restrict__ coef, float* __restrict__ ddisp, int accumulate,
                                                  float (&acc)[12]) {
  const int H = a.H, W = a.W;
  const long long plane = (long long)H * W, total = (long long)a.B * 3 * plane;
  for (long long p = first; p < plane; p += stride) {
    const int qy = (int)(p / W), qx = (int)(p % W);
    ReprojPix q;
    float tap[4][3], v[3];
    reproj_coords(a, disp, P, b, qy, qx, &q);
    reproj_sample(a, b, q, tap, v);
    const float gl1 = up((long long)b * plane + p) * ((1.f - a.w) / 3.f);
    // padded coordinates that map onto this pixel: itself, -1 (if it is 1), H (if it is H-2)
    int uy[3], ux[3], ny = 0, nx = 0;
    uy[ny++] = qy; if (qy == 1) uy[ny++] = -1; if (qy == H - 2) uy[ny++] = H;
    ux[nx++] = qx; if (qx == 1) ux[nx++] = -1; if (qx == W - 2) ux[nx++] = W;
    float g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float tv = a.tgt[((long long)b * 3 + c) * plane + p];
      const float* cf = coef + ((long long)b * 3 + c) * plane;
      float gs = 0.f;
      for (int i = 0; i < ny; ++i)
        for (int j = 0; j < nx; ++j)
          for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
              const int cy = uy[i] + dy, cx = ux[j] + dx;     // window centre
              if (cy < 0 || cy >= H || cx < 0 || cx >= W) continue;
              const long long k = (long long)cy * W + cx;
              gs += (cf[k] + 2.f * v[c] * cf[total + k] + tv * cf[2 * total + k]) / 9.f;
            }
      const float e = tv - v[c];
      g[c] = gs - gl1 * (e > 0.f ? 1.f : (e < 0.f ? -1.f : 0.f));
    }
    const float fx0 = floorf(q.ix), fy0 = floorf(q.iy);
    const float wx1 = q.ix - fx0, wx0 = (fx0 + 1.f) - q.ix, wy1 = q.iy - fy0, wy0 = (fy0 + 1.f) - q.iy;
    float gix = 0.f, giy = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      gix += g[c] * (-tap[0][c] * wy0 + tap[1][c] * wy0 - tap[2][c] * wy1 + tap[3][c] * wy1);
      giy += g[c] * (-tap[0][c] * wx0 - tap[1][c] * wx1 + tap[2][c] * wx0 + tap[3][c] * wx1);
    }
    // xn = (px / (W-1) - 0.5) * 2, px = c0 / z
    const float gpx = gix * q.mx * 2.f / (float)(W - 1), gpy = giy * q.my * 2.f / (float)(H - 1);
    const float dc0 = gpx / q.z, dc1 = gpy / q.z;
    const float dc2 = -(gpx * q.c0 + gpy * q.c1) / (q.z * q.z);
    const float p0 = q.depth * q.ray[0], p1 = q.depth * q.ray[1], p2 = q.depth * q.ray[2];
    const float dp0 = P[0] * dc0 + P[4] * dc1 + P[8] * dc2;
    const float dp1 = P[1] * dc0 + P[5] * dc1 + P[9] * dc2;
    const float dp2 = P[2] * dc0 + P[6] * dc1 + P[10] * dc2;
    float dd = dp0 * q.ray[0] + dp1 * q.ray[1] + dp2 * q.ray[2];
    if (a.disp_mode) dd = -dd * q.depth * q.depth * a.d_span;      // depth = 1 / (d_lo + d_span * disp)
    float* o = ddisp + (long long)b * plane + p;
    *o = accumulate ? *o + dd : dd;
    acc[0] += dc0 * p0; acc[1] += dc0 * p1; acc[2] += dc0 * p2; acc[3] += dc0;
    acc[4] += dc1 * p0; acc[5] += dc1 * p1; acc[6] += dc1 * p2; acc[7] += dc1;
    acc[8] += dc2 * p0; acc[9] += dc2 * p1; acc[10] += dc2 * p2; acc[11] += dc2;
  }
}

static inline int rp_blocks(long long total, int cap) {
  long long b = (total + 255) / 256;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}
static inline int reproj_blocks(int h, int w) { return rp_blocks((long long)h * w, 64); }

static inline int fill_reproj_args(ReprojArgs* a, const float* tgt, const float* ref, const float* disp, const float* K, const float* invK,
                                   const float* T, int B, int H, int W, int align, int disp_mode, float d_lo, float d_span, float eps, float w) {
  DN_REQUIRE(tgt && ref && B > 0 && H >= 2 && W >= 2, DN_ERR_BAD_ARG, "reproj: bad argument (needs H, W >= 2)");
  DN_REQUIRE((align == 0 || align == 1) && (disp_mode == 0 || disp_mode == 1), DN_ERR_BAD_ARG, "reproj: align %d / disp_mode %d", align, disp_mode);
  a->tgt = tgt; a->ref = ref; a->disp = disp; a->K = K; a->invK = invK; a->T = T;
  a->B = B; a->H = H; a->W = W; a->align = align; a->disp_mode = disp_mode; a->d_lo = d_lo; a->d_span = d_span; a->eps = eps; a->w = w;
  return DN_OK;
}

}  // namespace dn
