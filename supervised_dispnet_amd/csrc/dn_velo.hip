// Velodyne clouds -> sparse depth maps for prepare_train_data.py: generate_depth_map of the reference's
// data/kitti_raw_loader.py:243-300 (the algorithm of kitti_eval/depth_evaluation_utils.py:173-215) for a batch of frames in one call.
//   per point (x, y, z, .) with x >= 0:  p_i = ((M[i][0] * x + M[i][1] * y) + M[i][2] * z) + M[i][3] in fp64, no contraction;
//   u = p_0 / p_2, v = p_1 / p_2 (IEEE);  col = rint(u) - 1, row = rint(v) - 1 (half to even, np.round);
//   kept iff col >= 0, row >= 0, col < lim_w, row < lim_h (a NaN or inf fails);  depth = p_2;
//   key = row * (w - 1) + col - 1: the reference's sub2ind, which is NOT a pixel index -- (r, 0) and (r - 1, w - 1) share a key.
// The map: every hit pixel takes the depth of the LAST point on it; every key hit more than once then writes the MINIMUM depth of its
// group at the pixel of the group's FIRST point; negative values become 0; one fp64 -> fp32 rounding at the store.
// Three launches, ordered by the stream (so agent scope and relaxed order suffice):
//   velo_init_kernel     the tables: last point per pixel = -1, first point per key = INT_MAX, count per key = 0, depth per key = ~0;
//   velo_scatter_kernel  one thread per point, one float4 load, no-return atomics: max of the point index per pixel; min of the point
//                        index, add of a count and a 64-bit min of the depth's order-preserving bit pattern per key;
//   velo_resolve_kernel  one thread per pixel: the depth of its last point (projected again, the same arithmetic), replaced by the key's
//                        minimum when the key's first point is on this pixel.
// Every atomic is an integer min, max or add: the tables, and with them the map, do not depend on the order in which points arrive, so
// the result is deterministic and independent of scheduling.  No LDS.
#include "dn_internal.h"

#pragma clang fp contract(off)

namespace dn {

constexpr int kVeloThreads = 256;

struct VeloTables {               // views into the caller's workspace
  unsigned long long* kdepth;     // [B][nkeys] flipped bit pattern of the smallest depth
  int* last;                      // [B][h * w] largest point index on the pixel, -1: none
  int* kfirst;                    // [B][nkeys] smallest point index of the key
  int* kcount;                    // [B][nkeys] points of the key
};

// keys run from -1 (pixel (0, 0)) to (h - 1) * (w - 1) + w - 2: h * (w - 1) + 1 slots, slot = key + 1
static __host__ __device__ __forceinline__ long long velo_keys(int h, int w) { return (long long)h * (w - 1) + 1; }

static __host__ __device__ __forceinline__ VeloTables velo_tables(void* ws, long long B, int h, int w) {
  const long long nk = B * velo_keys(h, w), np = B * h * w;
  VeloTables t;
  t.kdepth = reinterpret_cast<unsigned long long*>(ws);
  t.last = reinterpret_cast<int*>(t.kdepth + nk);
  t.kfirst = t.last + np;
  t.kcount = t.kfirst + nk;
  return t;
}

// doubles order like these unsigned patterns (negative values below positive ones)
static __device__ __forceinline__ unsigned long long depth_key(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
static __device__ __forceinline__ double key_depth(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k));
}

// one point through the frame's 3 x 4 matrix -> inside the image?  (row, col, depth)
static __device__ __forceinline__ bool velo_project(const float4 pt, const double* __restrict__ m, int h, int w, double lim_h, double lim_w,
                                                    int* row, int* col, double* depth) {
  if (!(pt.x >= 0.f)) return false;
  const double x = (double)pt.x, y = (double)pt.y, z = (double)pt.z;
  const double p0 = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  const double p1 = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  const double p2 = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
  const double c = rint(p0 / p2) - 1.0, r = rint(p1 / p2) - 1.0;
  if (!(c >= 0.0 && r >= 0.0 && c < lim_w && r < lim_h)) return false;
  // Belt and braces: cannot fire, because the entry point refuses lim > size and the test above holds c < lim_w, r < lim_h.  Kept (two
  // compares per projection) so that the table indices below are bounded by what this function itself has tested.
  if (!(c < (double)w && r < (double)h)) return false;
  *row = (int)r;
  *col = (int)c;
  *depth = p2;
  return true;
}

__global__ void __launch_bounds__(kVeloThreads) velo_init_kernel(VeloTables t, long long npix, long long nkey) {
  const long long n = npix > nkey ? npix : nkey;
  for (long long i = blockIdx.x * (long long)kVeloThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kVeloThreads) {
    if (i < npix) t.last[i] = -1;
    if (i < nkey) {
      t.kdepth[i] = ~0ull;
      t.kfirst[i] = 0x7FFFFFFF;
      t.kcount[i] = 0;
    }
  }
}

__global__ void __launch_bounds__(kVeloThreads) velo_scatter_kernel(const float4* __restrict__ points, const long long* __restrict__ pt_off,
                                                                    const double* __restrict__ M, int B, int h, int w, double lim_h,
                                                                    double lim_w, long long total, VeloTables t) {
  const long long gi = blockIdx.x * (long long)kVeloThreads + threadIdx.x;
  if (gi >= total || gi < pt_off[0] || gi >= pt_off[B]) return;
  int lo = 0, hi = B;                                      // the frame with pt_off[lo] <= gi < pt_off[lo + 1]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (pt_off[mid] <= gi) lo = mid; else hi = mid;
  }
  const int b = lo;
  const long long local = gi - pt_off[b];
  if (local < 0 || local > 0x7FFFFFFE) return;
  int row, col;
  double depth;
  if (!velo_project(points[gi], M + 12 * b, h, w, lim_h, lim_w, &row, &col, &depth)) return;
  const int idx = (int)local;
  const long long pix = ((long long)b * h + row) * w + col;
  const long long key = (long long)b * velo_keys(h, w) + ((long long)row * (w - 1) + col);     // slot = key + 1
  __hip_atomic_fetch_max(t.last + pix, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_min(t.kfirst + key, idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_add(t.kcount + key, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_min(t.kdepth + key, depth_key(depth), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(kVeloThreads) velo_resolve_kernel(const float4* __restrict__ points, const long long* __restrict__ pt_off,
                                                                    const double* __restrict__ M, int B, int h, int w, double lim_h,
                                                                    double lim_w, VeloTables t, float* __restrict__ out) {
  const long long npix = (long long)B * h * w;
  const long long p = blockIdx.x * (long long)kVeloThreads + threadIdx.x;
  if (p >= npix) return;
  const int col = (int)(p % w), row = (int)((p / w) % h), b = (int)(p / ((long long)h * w));
  float v = 0.f;
  const int li = t.last[p];
  if (li >= 0) {
    const double* m = M + 12 * b;
    const float4* pts = points + pt_off[b];
    int r, c;
    double depth = 0.0;
    velo_project(pts[li], m, h, w, lim_h, lim_w, &r, &c, &depth);        // the point that put li here: inside, on this pixel
    const long long key = (long long)b * velo_keys(h, w) + ((long long)row * (w - 1) + col);
    if (t.kcount[key] > 1) {
      // the key's first point is on this pixel, unless the key is one that two pixels share (column 0 and column w - 1)
      bool here = true;
      if (col == 0 || col == w - 1) {
        double d;
        here = velo_project(pts[t.kfirst[key]], m, h, w, lim_h, lim_w, &r, &c, &d) && r == row && c == col;
      }
      if (here) depth = key_depth(t.kdepth[key]);
    }
    v = depth < 0.0 ? 0.f : (float)depth;
  }
  out[p] = v;
}

static inline bool velo_shape_ok(long long B, int h, int w, long long total) {
  return B > 0 && B <= 65535 && h > 0 && w >= 2 && total >= 0 && total <= 0x7FFFFFFELL && B * h * w <= 0x7FFFFFFFLL * 256;
}

}  // namespace dn

using namespace dn;

extern "C" {

size_t dn_velo_depth_workspace_bytes(int32_t B, int32_t h, int32_t w, int64_t total_points) {
  if (!velo_shape_ok(B, h, w, total_points)) return 0;
  const long long nk = (long long)B * velo_keys(h, w), np = (long long)B * h * w;
  return (size_t)(nk * 16 + np * 4);
}

int dn_velo_depth(const float* points, const int64_t* pt_off, int64_t total_points, const double* M, int32_t B, int32_t h, int32_t w,
                  double lim_h, double lim_w, void* workspace, size_t workspace_bytes, float* out, dn_stream_t stream) {
  DN_REQUIRE(velo_shape_ok(B, h, w, total_points), DN_ERR_BAD_ARG,
             "dn_velo_depth: bad shape (B = %d, h = %d, w = %d (>= 2), %lld points)", (int)B, (int)h, (int)w, (long long)total_points);
  DN_REQUIRE(pt_off && M && out && workspace && (points || total_points == 0), DN_ERR_BAD_ARG, "dn_velo_depth: null argument");
  DN_REQUIRE((reinterpret_cast<uintptr_t>(points) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace) & 7) == 0, DN_ERR_BAD_ARG,
             "dn_velo_depth: points must be 16-byte and the workspace 8-byte aligned");
  DN_REQUIRE(lim_h > 0.0 && lim_w > 0.0 && lim_h <= (double)h && lim_w <= (double)w, DN_ERR_BAD_ARG,
             "dn_velo_depth: the bounds %g x %g must lie in (0, %d] x (0, %d]: a point past the map has no pixel", lim_h, lim_w, (int)h,
             (int)w);
  DN_REQUIRE(workspace_bytes >= dn_velo_depth_workspace_bytes(B, h, w, total_points), DN_ERR_WORKSPACE,
             "dn_velo_depth: workspace of %zu bytes, %zu needed", workspace_bytes, dn_velo_depth_workspace_bytes(B, h, w, total_points));
  hipStream_t s = as_stream(stream);
  const VeloTables t = velo_tables(workspace, B, h, w);
  const long long nkey = (long long)B * velo_keys(h, w), npix = (long long)B * h * w;
  long long blocks = ((npix > nkey ? npix : nkey) + kVeloThreads - 1) / kVeloThreads;
  if (blocks > 4096) blocks = 4096;
  DN_LAUNCH(velo_init_kernel, dim3((unsigned)blocks), dim3(kVeloThreads), 0, s, t, npix, nkey);
  int rc = check_launch("velo_init_kernel");
  if (rc) return rc;
  if (total_points > 0) {
    DN_LAUNCH(velo_scatter_kernel, dim3((unsigned)((total_points + kVeloThreads - 1) / kVeloThreads)), dim3(kVeloThreads), 0, s,
              reinterpret_cast<const float4*>(points), (const long long*)pt_off, M, (int)B, (int)h, (int)w, lim_h, lim_w,
              (long long)total_points, t);
    rc = check_launch("velo_scatter_kernel");
    if (rc) return rc;
  }
  DN_LAUNCH(velo_resolve_kernel, dim3((unsigned)((npix + kVeloThreads - 1) / kVeloThreads)), dim3(kVeloThreads), 0, s,
            reinterpret_cast<const float4*>(points), (const long long*)pt_off, M, (int)B, (int)h, (int)w, lim_h, lim_w, t, out);
  return check_launch("velo_resolve_kernel");
}

}  // extern "C"
