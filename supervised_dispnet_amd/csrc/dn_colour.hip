// monodepth2's colour jitter of the shard loader on the device: per sample a random order of brightness, contrast,
// saturation and hue, each defined by Pillow's own 8-bit arithmetic (what torchvision's ColorJitter runs on PIL images), fused with the
// loader's flip and normalise.  Equality with the host chain (data.colour_jitter_u8, then data.Transform.apply) is the contract.
//   dn_colour_jitter_sums            per frame DN_IMAGE_CHUNKS partial sums of the luma the contrast step will see: the operations that
//                                    precede contrast in the sample's order are applied in registers, the luma is summed as integers
//                                    (64-bit), so the sum has no order.  A sample that is not jittered does nothing.
//   dn_colour_jitter_normalize_flip  per pixel the whole chain (m from the sums), then dn_u8_normalize_flip's flip and arithmetic; the
//                                    augmented fp32 batch and, when asked, the plain one from the same read of the bytes.
//   dn_colour_jitter_u8              the same chain with a uint8 result and no flip (feeds dn_scale_crop_u8).
// Two launches per batch for all N * B frames.  The order of a frame's operations is the same for every thread of a block (blockIdx.y is
// the frame), so the chain branches on scalar registers.  W % 4 == 0: a thread owns 4 consecutive pixels of a row (three aligned dwords);
// any other width: one pixel per thread.
#include "dn_internal.h"

#pragma clang fp contract(off)                           // Pillow's blend is a rounded product and a rounded sum, never an FMA

namespace dn {

constexpr int kColThreads = 256;

struct ColourParams {                                    // one row of the per-sample table, DN_COLOUR_PARAMS int32
  int on, order;                                         // order: 2 bits per step, first step in the low bits
  float b, c, s;
  int shift;
};

static __device__ __forceinline__ ColourParams colour_params(const int* __restrict__ params, int sample) {
  const int* p = params + (long long)sample * DN_COLOUR_PARAMS;
  ColourParams q;
  q.on = p[0];
  q.order = p[1];
  q.b = __int_as_float(p[2]);
  q.c = __int_as_float(p[3]);
  q.s = __int_as_float(p[4]);
  q.shift = p[5] & 255;
  return q;
}

static __device__ __forceinline__ int col_luma(int r, int g, int b) {   // Pillow's RGB -> L
  return (int)((19595u * (unsigned)r + 38470u * (unsigned)g + 7471u * (unsigned)b + 0x8000u) >> 16);
}

// Image.blend(a, x, alpha): uint8(clip(fp32(a) + alpha * (fp32(x) - fp32(a)), 0, 255)).  Plain operators under this file's contract(off):
// __fmul_rn / __fadd_rn are inline functions of a header compiled with contraction on, and their product and sum fuse after inlining
// (135 + 0.8f * (0 - 135) is 27 with the rounded product 108 and 26 fused).
static __device__ __forceinline__ int col_blend(float a, float alpha, int x) {
  const float d = (float)x - a;
  const float prod = alpha * d;
  const float t = a + prod;
  return (int)fminf(fmaxf(t, 0.f), 255.f);
}

static __device__ __forceinline__ int col_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's rgb2hsv_row, the hue moved by `shift` mod 256, Pillow's hsv2rgb
static __device__ __forceinline__ void col_hue(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {                                        // (black is grey: no division by max == 0)
    const float cr = (float)(mx - mn);
    const float s = __fdiv_rn(cr, (float)mx);
    const float rc = __fdiv_rn((float)(mx - r), cr), gc = __fdiv_rn((float)(mx - g), cr), bc = __fdiv_rn((float)(mx - b), cr);
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;              // in [5/6, 11/6]: fmod(x, 1.0) == x - floor(x), exactly
    h = (float)(x - floor(x));
    H = col_clip8((int)((double)h * 255.0));
    S = col_clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double h6 = (double)H * 6.0 / 255.0;
  const double fl = floor(h6);
  const float f = (float)(h6 - fl);
  const float fs = (float)((double)S / 255.0);
  const double v = (double)V;
  const int p = col_clip8((int)round(v * (1.0 - (double)fs)));
  const int q = col_clip8((int)round(v * (1.0 - (double)(fs * f))));
  const int t = col_clip8((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))));
  switch ((int)fl % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// one step of the chain on one pixel; op and the factors are the same for the whole block
static __device__ __forceinline__ void col_step(int op, const ColourParams& q, float m, int& r, int& g, int& b) {
  if (op == 0) {
    r = col_blend(0.f, q.b, r);
    g = col_blend(0.f, q.b, g);
    b = col_blend(0.f, q.b, b);
  } else if (op == 1) {
    r = col_blend(m, q.c, r);
    g = col_blend(m, q.c, g);
    b = col_blend(m, q.c, b);
  } else if (op == 2) {
    const float L = (float)col_luma(r, g, b);
    r = col_blend(L, q.s, r);
    g = col_blend(L, q.s, g);
    b = col_blend(L, q.s, b);
  } else {
    col_hue(r, g, b, q.shift);
  }
}

// the steps in front of contrast (for the sums) or all four (nsteps = 4)
static __device__ __forceinline__ void col_chain(const ColourParams& q, int nsteps, float m, int& r, int& g, int& b) {
  for (int k = 0; k < nsteps; ++k) col_step((q.order >> (2 * k)) & 3, q, m, r, g, b);
}

static __device__ __forceinline__ int col_steps_before_contrast(int order) {
  int k = 0;
  while (k < 4 && ((order >> (2 * k)) & 3) != 1) ++k;
  return k;
}

static __device__ __forceinline__ void unpack12(const uint32_t* __restrict__ p, int* px) {
  const uint32_t w0 = p[0], w1 = p[1], w2 = p[2];
  px[0] = w0 & 255; px[1] = (w0 >> 8) & 255; px[2] = (w0 >> 16) & 255; px[3] = w0 >> 24;
  px[4] = w1 & 255; px[5] = (w1 >> 8) & 255; px[6] = (w1 >> 16) & 255; px[7] = w1 >> 24;
  px[8] = w2 & 255; px[9] = (w2 >> 8) & 255; px[10] = (w2 >> 16) & 255; px[11] = w2 >> 24;
}

// ---- partial luma sums.  grid (DN_IMAGE_CHUNKS, N * B); VEC: npix % 4 == 0 and 4-byte aligned frames, a thread takes 4 pixels per turn
template <bool VEC>
__global__ void __launch_bounds__(kColThreads) colour_sums_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ params, int B,
                                                                  long long npix, unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long ssum[kColThreads];
  const int frame = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x, tid = threadIdx.x;
  const ColourParams q = colour_params(params, frame % B);
  if (!q.on) return;
  const int nsteps = col_steps_before_contrast(q.order);
  const uint8_t* f = frames + (long long)frame * npix * 3;
  unsigned long long s = 0;
  if (VEC) {
    const long long ng = npix >> 2;
    const long long lo = ng * chunk / nchunk, hi = ng * (chunk + 1) / nchunk;
    for (long long i = lo + tid; i < hi; i += kColThreads) {
      int px[12];
      unpack12(reinterpret_cast<const uint32_t*>(f + i * 12), px);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
        col_chain(q, nsteps, 0.f, r, g, b);
        s += (unsigned)col_luma(r, g, b);
      }
    }
  } else {
    const long long lo = npix * chunk / nchunk, hi = npix * (chunk + 1) / nchunk;
    for (long long i = lo + tid; i < hi; i += kColThreads) {
      int r = f[i * 3], g = f[i * 3 + 1], b = f[i * 3 + 2];
      col_chain(q, nsteps, 0.f, r, g, b);
      s += (unsigned)col_luma(r, g, b);
    }
  }
  ssum[tid] = s;
  __syncthreads();
  for (int o = kColThreads / 2; o > 0; o >>= 1) {
    if (tid < o) ssum[tid] += ssum[tid + o];
    __syncthreads();
  }
  if (tid == 0) partial[(long long)frame * nchunk + chunk] = ssum[0];
}

// ---- the chain and the epilogue.  grid (blocks over the frame's pixels, N * B).  U8: uint8 [N][B][H][W][3] out, no flip;
// else fp32 [N][B][3][H][W] out (and plain, unless nullptr) with the flip and (u8 / 255 - mean) / std.
template <bool VEC, bool U8>
__global__ void __launch_bounds__(kColThreads) colour_apply_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ flip,
                                                                   const int* __restrict__ params,
                                                                   const unsigned long long* __restrict__ partial, int B, int H, int W,
                                                                   float m0, float m1, float m2, float s0, float s1, float s2,
                                                                   float* __restrict__ out, float* __restrict__ plain,
                                                                   uint8_t* __restrict__ out_u8) {
  __shared__ unsigned long long ssum[DN_IMAGE_CHUNKS];
  const int frame = blockIdx.y, sample = frame % B, tid = threadIdx.x;
  const ColourParams q = colour_params(params, sample);
  const long long npix = (long long)H * W;
  float m = 0.f;
  if (q.on) {                                            // block-uniform: every thread meets the barrier or none does
    if (tid < DN_IMAGE_CHUNKS) ssum[tid] = partial[(long long)frame * DN_IMAGE_CHUNKS + tid];
    __syncthreads();
    unsigned long long total = 0;
#pragma unroll 4
    for (int k = 0; k < DN_IMAGE_CHUNKS; ++k) total += ssum[k];
    m = (float)(int)((double)total / (double)npix + 0.5);
  }
  const bool fl = !U8 && flip != nullptr && flip[sample] != 0;
  const uint8_t* f = frames + (long long)frame * npix * 3;
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  const long long obase = (long long)frame * npix * 3;   // the frame's first element in every output
  if (VEC) {
    const int W4 = W >> 2;
    const long long ng = (long long)H * W4;
    for (long long i = blockIdx.x * (long long)kColThreads + tid; i < ng; i += (long long)gridDim.x * kColThreads) {
      const int x0 = (int)(i % W4) * 4, y = (int)(i / W4);            // first OUTPUT pixel of the group
      const int sx = fl ? W - 4 - x0 : x0;                            // first source pixel (reversed inside when flipped)
      int px[12], ax[12];
      unpack12(reinterpret_cast<const uint32_t*>(f + ((long long)y * W + sx) * 3), px);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        int r = px[3 * k], g = px[3 * k + 1], b = px[3 * k + 2];
        if (q.on) col_chain(q, 4, m, r, g, b);
        ax[3 * k] = r; ax[3 * k + 1] = g; ax[3 * k + 2] = b;
      }
      if (U8) {
        uint32_t* o = reinterpret_cast<uint32_t*>(out_u8 + obase + ((long long)y * W + x0) * 3);
        o[0] = (uint32_t)ax[0] | ((uint32_t)ax[1] << 8) | ((uint32_t)ax[2] << 16) | ((uint32_t)ax[3] << 24);
        o[1] = (uint32_t)ax[4] | ((uint32_t)ax[5] << 8) | ((uint32_t)ax[6] << 16) | ((uint32_t)ax[7] << 24);
        o[2] = (uint32_t)ax[8] | ((uint32_t)ax[9] << 8) | ((uint32_t)ax[10] << 16) | ((uint32_t)ax[11] << 24);
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          float4 oa, op;
          float *pa = &oa.x, *pp = &op.x;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const int sk = fl ? 3 - k : k;
            pa[k] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)ax[sk * 3 + c], 255.f), mean[c]), stdv[c]);
            pp[k] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)px[sk * 3 + c], 255.f), mean[c]), stdv[c]);
          }
          const long long o = obase + (long long)c * npix + (long long)y * W + x0;
          *reinterpret_cast<float4*>(out + o) = oa;
          if (plain != nullptr) *reinterpret_cast<float4*>(plain + o) = op;
        }
      }
    }
  } else {
    for (long long i = blockIdx.x * (long long)kColThreads + tid; i < npix; i += (long long)gridDim.x * kColThreads) {
      const int x = (int)(i % W), y = (int)(i / W);
      const int sx = fl ? W - 1 - x : x;
      const uint8_t* p = f + ((long long)y * W + sx) * 3;
      const int pr = p[0], pg = p[1], pb = p[2];
      int r = pr, g = pg, b = pb;
      if (q.on) col_chain(q, 4, m, r, g, b);
      if (U8) {
        uint8_t* o = out_u8 + obase + i * 3;
        o[0] = (uint8_t)r; o[1] = (uint8_t)g; o[2] = (uint8_t)b;
      } else {
        const int av[3] = {r, g, b}, pv[3] = {pr, pg, pb};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const long long o = obase + (long long)c * npix + i;
          out[o] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)av[c], 255.f), mean[c]), stdv[c]);
          if (plain != nullptr) plain[o] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)pv[c], 255.f), mean[c]), stdv[c]);
        }
      }
    }
  }
}

// blocks per frame: about 8192 over all frames (256 CUs x 8 blocks x 4 rounds), the rest of a frame by grid stride
static inline unsigned colour_blocks(long long items, long long frames) {
  const long long b = (items + kColThreads - 1) / kColThreads;
  const long long cap = (8192 + frames - 1) / frames;
  return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

static int colour_check(const char* who, const void* frames, const void* params, int32_t N, int32_t B, int32_t H, int32_t W) {
  DN_REQUIRE(frames && params && N > 0 && B > 0 && H > 0 && W > 0, DN_ERR_BAD_ARG, "%s: bad argument", who);
  DN_REQUIRE((long long)N * B <= 65535, DN_ERR_UNSUPPORTED, "%s: %lld frames are too many for one launch", who, (long long)N * B);
  return DN_OK;
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_colour_jitter_sums(const uint8_t* frames, const int32_t* params, int32_t N, int32_t B, int32_t H, int32_t W, uint64_t* sum_ws,
                          dn_stream_t stream) {
  const int rc = colour_check("dn_colour_jitter_sums", frames, params, N, B, H, W);
  if (rc) return rc;
  DN_REQUIRE(sum_ws, DN_ERR_WORKSPACE, "dn_colour_jitter_sums: missing workspace");
  const long long npix = (long long)H * W;
  const dim3 grid(DN_IMAGE_CHUNKS, (unsigned)(N * B));
  const bool vec = (npix & 3) == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0;
  if (vec) {
    DN_LAUNCH(colour_sums_kernel<true>, grid, dim3(kColThreads), 0, as_stream(stream), frames, (const int*)params, (int)B, npix,
              (unsigned long long*)sum_ws);
  } else {
    DN_LAUNCH(colour_sums_kernel<false>, grid, dim3(kColThreads), 0, as_stream(stream), frames, (const int*)params, (int)B, npix,
              (unsigned long long*)sum_ws);
  }
  set_last_kernel("dn::colour_sums_kernel<%s>", vec ? "true" : "false");
  return check_launch("colour_sums_kernel");
}

int dn_colour_jitter_normalize_flip(const uint8_t* frames, const uint8_t* flip, const int32_t* params, const uint64_t* sum_ws, int32_t N,
                                    int32_t B, int32_t H, int32_t W, const float* mean_host, const float* std_host, float* out, float* plain,
                                    dn_stream_t stream) {
  const int rc = colour_check("dn_colour_jitter_normalize_flip", frames, params, N, B, H, W);
  if (rc) return rc;
  DN_REQUIRE(sum_ws && mean_host && std_host && out && out != plain, DN_ERR_BAD_ARG, "dn_colour_jitter_normalize_flip: bad argument");
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(plain) & 15) == 0;
  const long long items = vec ? (long long)H * (W >> 2) : (long long)H * W;
  const dim3 grid(colour_blocks(items, (long long)N * B), (unsigned)(N * B));
  if (vec) {
    DN_LAUNCH((colour_apply_kernel<true, false>), grid, dim3(kColThreads), 0, as_stream(stream), frames, flip, (const int*)params,
              (const unsigned long long*)sum_ws, (int)B, (int)H, (int)W, mean_host[0], mean_host[1], mean_host[2], std_host[0], std_host[1],
              std_host[2], out, plain, (uint8_t*)nullptr);
  } else {
    DN_LAUNCH((colour_apply_kernel<false, false>), grid, dim3(kColThreads), 0, as_stream(stream), frames, flip, (const int*)params,
              (const unsigned long long*)sum_ws, (int)B, (int)H, (int)W, mean_host[0], mean_host[1], mean_host[2], std_host[0], std_host[1],
              std_host[2], out, plain, (uint8_t*)nullptr);
  }
  set_last_kernel("dn::colour_apply_kernel<%s, false>", vec ? "true" : "false");
  return check_launch("colour_apply_kernel");
}

int dn_colour_jitter_u8(const uint8_t* frames, const int32_t* params, const uint64_t* sum_ws, int32_t N, int32_t B, int32_t H, int32_t W,
                        uint8_t* out, dn_stream_t stream) {
  const int rc = colour_check("dn_colour_jitter_u8", frames, params, N, B, H, W);
  if (rc) return rc;
  DN_REQUIRE(sum_ws && out && out != frames, DN_ERR_BAD_ARG, "dn_colour_jitter_u8: bad argument (not in place)");
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(frames) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0;
  const long long items = vec ? (long long)H * (W >> 2) : (long long)H * W;
  const dim3 grid(colour_blocks(items, (long long)N * B), (unsigned)(N * B));
  if (vec) {
    DN_LAUNCH((colour_apply_kernel<true, true>), grid, dim3(kColThreads), 0, as_stream(stream), frames, (const uint8_t*)nullptr,
              (const int*)params, (const unsigned long long*)sum_ws, (int)B, (int)H, (int)W, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, (float*)nullptr,
              (float*)nullptr, out);
  } else {
    DN_LAUNCH((colour_apply_kernel<false, true>), grid, dim3(kColThreads), 0, as_stream(stream), frames, (const uint8_t*)nullptr,
              (const int*)params, (const unsigned long long*)sum_ws, (int)B, (int)H, (int)W, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f, (float*)nullptr,
              (float*)nullptr, out);
  }
  set_last_kernel("dn::colour_apply_kernel<%s, true>", vec ? "true" : "false");
  return check_launch("colour_apply_kernel");
}

}  // extern "C"
