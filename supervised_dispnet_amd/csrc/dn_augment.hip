// Random scale-and-crop augmentation of the shard loader on the device: the reference's
// custom_transforms.RandomScaleCrop (:73-113) -- scipy.misc.imresize of every image of a sample to (sh, sw) >= (H, W), a crop back to
// H x W at (oy, ox), the same for the ground-truth depth -- fused with the loader's flip and normalise.  Equality with the host chain
// (data.Transform(scale_crop=True)) is the contract, not a tolerance: every step is integer or fixed fp32 / fp64 arithmetic.
//   dn_scale_crop_minmax   DN_IMAGE_CHUNKS partial (min, max) pairs per uint8 frame (over all three channels) and per fp32 depth map, one
//                          launch for both; the consumers fold them (min / max reductions: no order, no float atomics).
//   dn_scale_crop_u8       per 16 x 64 output tile: stage the (at most 18 x 66 pixel) input window the tile's taps read into LDS,
//                          mirrored in the index when the sample is flipped and byte-scaled on load (a 256-entry table per frame);
//                          horizontal pass into uint8 rows in LDS; vertical pass from LDS; (u8 / 255 - mean) / std; coalesced fp32 rows
//                          per channel plane.  The uint8 intermediate between the passes is Pillow's and part of the contract.
//   dn_scale_crop_depth    the same on the one-channel fp32 map (byte-scale by arithmetic on load), then fp32(fp64(u8) / 255.0 * fp64(max)).
// The host builds the windowed coefficient rows (supervised_dispnet_amd/inference.py: scale_crop_rows): only the W crop columns and the
// H crop rows of each sample, {first input index, k0, k1, k2} -- upscaling has support 1, so Pillow never has more than 3 taps.
#include "dn_internal.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kAugThreads = 256;
constexpr int kATileH = 16, kATileW = 64;                // output tile
constexpr int kAInH = kATileH + 2, kAInW = kATileW + 2;  // input window: the first tap of a tile's last row / column + 2 more
constexpr int kAPrecBits = 22;                           // Pillow's PRECISION_BITS for 8-bit images (32 - 8 - 2)

static __device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// ---- partial (min, max): blockIdx.y < n_frames is a uint8 frame of 3 * HW bytes, the rest are fp32 maps of HW floats
__global__ void __launch_bounds__(kAugThreads) scale_crop_minmax_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ depth,
                                                                        int n_frames, long long HW, int* __restrict__ mm_u8,
                                                                        float* __restrict__ mm_f32) {
  __shared__ float smn[kAugThreads], smx[kAugThreads];
  const int img = blockIdx.y, chunk = blockIdx.x, nchunk = gridDim.x, tid = threadIdx.x;
  if (img < n_frames) {
    // bytes as integers; exact in fp32, so the two kinds share the reduction below
    const long long n = 3 * HW;
    const long long lo = n * chunk / nchunk, hi = n * (chunk + 1) / nchunk;
    const uint8_t* p = frames + (long long)img * n + lo;
    const long long len = hi - lo;
    int mn = 255, mx = 0;
    const int head = (int)min(len, (long long)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3));
    if (tid < head) mn = mx = p[tid];
    const long long nwords = (len - head) / 4;
    const uint32_t* pw = reinterpret_cast<const uint32_t*>(p + head);
    for (long long i = tid; i < nwords; i += kAugThreads) {
      const uint32_t v = pw[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int a = (int)((v >> (8 * k)) & 255u);
        mn = min(mn, a);
        mx = max(mx, a);
      }
    }
    const long long t = head + 4 * nwords + tid;
    if (t < len) {
      const int a = p[t];
      mn = min(mn, a);
      mx = max(mx, a);
    }
    smn[tid] = (float)mn;
    smx[tid] = (float)mx;
  } else {
    const long long lo = HW * chunk / nchunk, hi = HW * (chunk + 1) / nchunk;
    const float* p = depth + (long long)(img - n_frames) * HW;
    float mn = INFINITY, mx = -INFINITY;
    for (long long i = lo + tid; i < hi; i += kAugThreads) {
      const float v = p[i];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    smn[tid] = mn;
    smx[tid] = mx;
  }
  __syncthreads();
  for (int o = kAugThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      smn[tid] = fminf(smn[tid], smn[tid + o]);
      smx[tid] = fmaxf(smx[tid], smx[tid + o]);
    }
    __syncthreads();
  }
  if (tid == 0) {
    if (img < n_frames) {
      mm_u8[((long long)img * nchunk + chunk) * 2 + 0] = (int)smn[0];
      mm_u8[((long long)img * nchunk + chunk) * 2 + 1] = (int)smx[0];
    } else {
      mm_f32[((long long)(img - n_frames) * nchunk + chunk) * 2 + 0] = smn[0];
      mm_f32[((long long)(img - n_frames) * nchunk + chunk) * 2 + 1] = smx[0];
    }
  }
}

// ---- the tile kernel.  T = uint8_t, C = 3: frames [N][B][H][W][3] -> fp32 [N][B][3][H][W];  T = float, C = 1: depth [B][H][W] -> [B][H][W].
// blockIdx.z = image (n * B + b); its sample b = z % B owns flip[b] and table rows [b][0, W) (columns) and [b][W, W + H) (rows).
// Every index read from the table is clamped into the staged window, so a table that is not Pillow's gives wrong pixels, never a read
// outside the frame.
template <typename T, int C>
__global__ void __launch_bounds__(kAugThreads) scale_crop_tile_kernel(const T* __restrict__ src, const uint8_t* __restrict__ flip,
                                                                      const void* __restrict__ minmax, const int* __restrict__ table, int B,
                                                                      int H, int W, float* __restrict__ out, float m0, float m1, float m2,
                                                                      float s0, float s1, float s2) {
  constexpr bool kDepth = std::is_same<T, float>::value;
  __shared__ int xt[kATileW][4];
  __shared__ int yt[kATileH][4];
  __shared__ float smm[DN_IMAGE_CHUNKS][2];
  __shared__ float flut[kDepth ? 256 : 1];               // depth: the value of every output byte
  __shared__ uint8_t lut[kDepth ? 1 : 256];              // frames: the byte-scale of every input byte
  __shared__ uint8_t win[kAInH][kAInW * C + 2];          // byte-scaled input window (row stride 200 / 68 bytes)
  __shared__ uint8_t mid[kAInH][kATileW * C];            // horizontal pass
  const int img = blockIdx.z, b = img % B, tid = threadIdx.x;
  const int r0 = blockIdx.y * kATileH, c0 = blockIdx.x * kATileW;
  const int nrow = min(kATileH, H - r0), ncol = min(kATileW, W - c0);
  const bool f = flip != nullptr && flip[b] != 0;

  // fold the partial (min, max) of this image; load the tile's table rows
  if (tid < DN_IMAGE_CHUNKS * 2) {
    const long long e = (long long)img * DN_IMAGE_CHUNKS * 2 + tid;
    smm[tid >> 1][tid & 1] = kDepth ? reinterpret_cast<const float*>(minmax)[e] : (float)reinterpret_cast<const int*>(minmax)[e];
  }
  const int* tb = table + (long long)b * (W + H) * 4;
  if (tid < ncol * 4) xt[tid >> 2][tid & 3] = tb[(long long)(c0 + (tid >> 2)) * 4 + (tid & 3)];
  if (tid < nrow * 4) yt[tid >> 2][tid & 3] = tb[(long long)(W + r0 + (tid >> 2)) * 4 + (tid & 3)];
  __syncthreads();
  float cmin = INFINITY, cmax = -INFINITY;
  for (int k = 0; k < DN_IMAGE_CHUNKS; ++k) {
    cmin = fminf(cmin, smm[k][0]);
    cmax = fmaxf(cmax, smm[k][1]);
  }
  // uint8(clip(fp32((fp32(a) - cmin) * fp32(255.0 / (cmax - cmin))) + 0.5f, 0, 255)), scale 1 for a constant image
  const float scale = (float)(cmax > cmin ? 255.0 / ((double)cmax - (double)cmin) : 1.0);
  if constexpr (kDepth) {
    flut[tid] = (float)((double)tid / 255.0 * (double)cmax);
  } else {
    const float t = __fadd_rn(__fmul_rn(__fsub_rn((float)tid, cmin), scale), 0.5f);
    lut[tid] = (uint8_t)fminf(fmaxf(t, 0.f), 255.f);
  }
  const int xlo = min(max(xt[0][0], 0), W - 1), ylo = min(max(yt[0][0], 0), H - 1);
  const int nin_r = min(nrow + 2, kAInH), nin_c = min(ncol + 2, kAInW);
  if constexpr (!kDepth) __syncthreads();                // lut is read below

  // stage the window: rows ylo .., columns xlo .. of the FLIPPED image (clamped at its last row / column: such taps have weight 0)
  const T* fr = src + (long long)img * H * W * C;
  for (int item = tid; item < nin_r * nin_c; item += kAugThreads) {
    const int rr = item / nin_c, cc = item % nin_c;
    const int y = min(ylo + rr, H - 1), xf = min(xlo + cc, W - 1);
    const int x = f ? W - 1 - xf : xf;
    const T* p = fr + ((long long)y * W + x) * C;
    if constexpr (kDepth) {
      const float t = __fadd_rn(__fmul_rn(__fsub_rn(p[0], cmin), scale), 0.5f);
      win[rr][cc] = (uint8_t)fminf(fmaxf(t, 0.f), 255.f);
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) win[rr][cc * C + c] = lut[p[c]];
    }
  }
  __syncthreads();

  // horizontal pass of the staged rows at the tile's columns: clip8((2^21 + sum k_i * in[first + i]) >> 22) -> uint8
  for (int item = tid; item < nin_r * ncol; item += kAugThreads) {
    const int rr = item / ncol, cc = item % ncol;
    const int x0 = min(max(xt[cc][0] - xlo, 0), nin_c - 1), x1 = min(x0 + 1, nin_c - 1), x2 = min(x0 + 2, nin_c - 1);
    const int k0 = xt[cc][1], k1 = xt[cc][2], k2 = xt[cc][3];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const int acc = (1 << (kAPrecBits - 1)) + k0 * (int)win[rr][x0 * C + c] + k1 * (int)win[rr][x1 * C + c] + k2 * (int)win[rr][x2 * C + c];
      mid[rr][cc * C + c] = (uint8_t)aug_clip8(acc >> kAPrecBits);
    }
  }
  __syncthreads();

  // vertical pass from LDS; column fastest, so every wave writes 256 contiguous bytes of one channel plane
  const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
  for (int item = tid; item < nrow * C * ncol; item += kAugThreads) {
    const int cc = item % ncol, c = (item / ncol) % C, gr = item / (C * ncol);
    const int y0 = min(max(yt[gr][0] - ylo, 0), nin_r - 1), y1 = min(y0 + 1, nin_r - 1), y2 = min(y0 + 2, nin_r - 1);
    const int acc = (1 << (kAPrecBits - 1)) + yt[gr][1] * (int)mid[y0][cc * C + c] + yt[gr][2] * (int)mid[y1][cc * C + c] +
                    yt[gr][3] * (int)mid[y2][cc * C + c];
    const int v = aug_clip8(acc >> kAPrecBits);
    const long long o = (((long long)img * C + c) * H + r0 + gr) * W + c0 + cc;
    if constexpr (kDepth) {
      out[o] = flut[v];
    } else {
      out[o] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)v, 255.f), mean[c]), stdv[c]);
    }
  }
}

// host-side argument checks shared by the two tile entry points: nothing is launched unless every sample's scaled size covers the crop
static int scale_crop_check(const char* who, int32_t B, int32_t H, int32_t W, const int32_t* scaled_hw_host, int32_t max_taps, dim3* grid,
                            long long images) {
  DN_REQUIRE(B > 0 && H > 0 && W > 0 && scaled_hw_host, DN_ERR_BAD_ARG, "%s: bad argument", who);
  DN_REQUIRE(max_taps >= 1 && max_taps <= DN_SCALE_CROP_TAPS, DN_ERR_BAD_ARG,
             "%s: %d taps per output, the table rows hold %d (a scaled axis shorter than the input? upscaling never needs more)", who,
             (int)max_taps, DN_SCALE_CROP_TAPS);
  for (int b = 0; b < B; ++b)
    DN_REQUIRE(scaled_hw_host[2 * b] >= H && scaled_hw_host[2 * b + 1] >= W, DN_ERR_BAD_ARG,
               "%s: sample %d is scaled to %d x %d, smaller than the %d x %d crop", who, b, (int)scaled_hw_host[2 * b],
               (int)scaled_hw_host[2 * b + 1], (int)H, (int)W);
  *grid = dim3((unsigned)((W + kATileW - 1) / kATileW), (unsigned)((H + kATileH - 1) / kATileH), (unsigned)images);
  DN_REQUIRE(grid->y <= 65535 && images <= 65535, DN_ERR_UNSUPPORTED, "%s: H = %d or %lld images are too many for one launch", who, (int)H,
             images);
  return DN_OK;
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_scale_crop_minmax(const uint8_t* frames, const float* depth, int32_t N, int32_t B, int32_t H, int32_t W, int32_t* minmax_u8,
                         float* minmax_depth, dn_stream_t stream) {
  DN_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0 && (frames || depth), DN_ERR_BAD_ARG, "dn_scale_crop_minmax: bad argument");
  DN_REQUIRE((!frames || (N > 0 && minmax_u8)) && (!depth || minmax_depth), DN_ERR_WORKSPACE, "dn_scale_crop_minmax: missing workspace");
  const long long nf = frames ? (long long)N * B : 0, nd = depth ? B : 0;
  DN_REQUIRE(nf + nd <= 65535, DN_ERR_UNSUPPORTED, "dn_scale_crop_minmax: %lld images are too many for one launch", nf + nd);
  DN_LAUNCH(scale_crop_minmax_kernel, dim3(DN_IMAGE_CHUNKS, (unsigned)(nf + nd)), dim3(kAugThreads), 0, as_stream(stream), frames, depth,
            (int)nf, (long long)H * W, (int*)minmax_u8, minmax_depth);
  return check_launch("scale_crop_minmax_kernel");
}

int dn_scale_crop_u8(const uint8_t* frames, const uint8_t* flip, int32_t N, int32_t B, int32_t H, int32_t W, const int32_t* minmax_u8,
                     const int32_t* table, const int32_t* scaled_hw_host, int32_t max_taps, const float* mean_host, const float* std_host,
                     float* out, dn_stream_t stream) {
  DN_REQUIRE(frames && minmax_u8 && table && mean_host && std_host && out && N > 0, DN_ERR_BAD_ARG, "dn_scale_crop_u8: bad argument");
  dim3 grid;
  const int rc = scale_crop_check("dn_scale_crop_u8", B, H, W, scaled_hw_host, max_taps, &grid, (long long)N * B);
  if (rc) return rc;
  DN_LAUNCH((scale_crop_tile_kernel<uint8_t, 3>), grid, dim3(kAugThreads), 0, as_stream(stream), frames, flip, (const void*)minmax_u8,
            (const int*)table, (int)B, (int)H, (int)W, out, mean_host[0], mean_host[1], mean_host[2], std_host[0], std_host[1], std_host[2]);
  return check_launch("scale_crop_tile_kernel<uint8_t, 3>");
}

int dn_scale_crop_depth(const float* depth, const uint8_t* flip, int32_t B, int32_t H, int32_t W, const float* minmax_depth,
                        const int32_t* table, const int32_t* scaled_hw_host, int32_t max_taps, float* out, dn_stream_t stream) {
  DN_REQUIRE(depth && minmax_depth && table && out && depth != out, DN_ERR_BAD_ARG, "dn_scale_crop_depth: bad argument (not in place)");
  dim3 grid;
  const int rc = scale_crop_check("dn_scale_crop_depth", B, H, W, scaled_hw_host, max_taps, &grid, B);
  if (rc) return rc;
  DN_LAUNCH((scale_crop_tile_kernel<float, 1>), grid, dim3(kAugThreads), 0, as_stream(stream), depth, flip, (const void*)minmax_depth,
            (const int*)table, (int)B, (int)H, (int)W, out, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f);
  return check_launch("scale_crop_tile_kernel<float, 1>");
}

}  // extern "C"
