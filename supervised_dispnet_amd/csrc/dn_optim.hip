// The optimizers on the parameter arena: Adam (host- and device-side step counter) and SGD with momentum.  gfx950 only.
#include "dn_colreduce.h"

namespace dn {

// torch.optim.Adam (single-tensor formulation, amsgrad off): lerp for exp_avg, addcmul for exp_avg_sq,
// denom = sqrt(v)/sqrt(bc2) + eps, p -= (lr/bc1) * m / denom.
__global__ void __launch_bounds__(kThreads) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, long long n, float beta1, float beta2, float eps,
                                                        float weight_decay, float step_size, float bc2_sqrt, float grad_scale) {
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    float gi = g[i] * grad_scale;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    float mi = m[i], vi = v[i];
    mi = mi + (gi - mi) * (1.f - beta1);
    vi = vi * beta2 + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

// Graph-replayable form: the step counter lives on the device, so a captured launch sequence advances it by itself.
//   hyper = {lr, beta1, beta2} in double (what the host form receives); derived = {step_size, bc2_sqrt, beta1, beta2} in float
__global__ void adam_tick_kernel(int* __restrict__ step, const double* __restrict__ hyper, float* __restrict__ derived) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int t = step[0] + 1;
  step[0] = t;
  // beta^t by repeated squaring (<= 31 dependent multiplies; within an ulp or two of pow() in fp64, i.e. far below the fp32 the
  // corrections are handed on in): the device library's double pow() made this one-thread kernel take 115 us on the critical queue
  auto ipow = [](double b, int e) {
    double r = 1.0;
    while (e > 0) {
      if (e & 1) r *= b;
      b *= b;
      e >>= 1;
    }
    return r;
  };
  const double bc1 = 1.0 - ipow(hyper[1], t);
  const double bc2 = 1.0 - ipow(hyper[2], t);
  derived[0] = (float)(hyper[0] / bc1);
  derived[1] = (float)sqrt(bc2);
  derived[2] = (float)hyper[1];
  derived[3] = (float)hyper[2];
}

__global__ void __launch_bounds__(kThreads) adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, long long n, float eps,
                                                            float weight_decay, const float* __restrict__ derived, float grad_scale) {
  const float beta1 = derived[2], beta2 = derived[3], step_size = derived[0], bc2_sqrt = derived[1];
  for (long long i = blockIdx.x * (long long)kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    float gi = g[i] * grad_scale;
    const float pi = p[i];
    if (weight_decay != 0.f) gi += weight_decay * pi;
    float mi = m[i], vi = v[i];
    mi = mi + (gi - mi) * (1.f - beta1);
    vi = vi * beta2 + (1.f - beta2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    p[i] = pi - step_size * (mi / denom);
  }
}

// torch.optim.SGD (dampening 0, nesterov off, maximize off), fp32:
//   gi = g*grad_scale; if (wd != 0) gi += wd*p; b = momentum*buf + gi; buf = b; p = p - lr*b.
// torch creates the momentum buffer on the first step as a copy of the gradient; a zero-initialised buffer gives exactly that value
// (momentum*0 + gi == gi), so there is no step counter and no tick kernel here.  momentum == 0 is the same path: the buffer then holds
// the gradient and p follows torch's buffer-less form.  The multiply-adds are written as fmaf, so every caller (host- or device-side
// hyper-parameters, 16-byte or 4-byte lanes) executes the same three instructions per element whatever the compiler would contract.
__device__ __forceinline__ void sgd_update(float& p, const float g, float& b, const float lr, const float momentum,
                                           const float weight_decay, const float grad_scale) {
  float gi = g * grad_scale;
  if (weight_decay != 0.f) gi = fmaf(weight_decay, p, gi);
  const float bi = fmaf(momentum, b, gi);
  b = bi;
  p = fmaf(-lr, bi, p);
}

// Elements [0, n) of (p, g, buf) for the whole grid.  16-byte loads and stores (one global_load_dwordx4 per lane and operand: 1 KiB per
// wave instruction, the widest global access) where the three pointers sit at the same offset within 16 bytes -- always, for an arena and
// its bucket ranges: offset 0 -- after a scalar head of up to 3 elements; the <= 3 elements behind the last whole float4 are scalar too.
// Pointers that disagree in that offset (legal for the C ABI: any 4-byte alignment) take the scalar lane for every element.
__device__ __forceinline__ void sgd_range(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, const long long n,
                                          const float lr, const float momentum, const float weight_decay, const float grad_scale) {
  const long long tid = blockIdx.x * (long long)kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
  const uintptr_t ap = (uintptr_t)p, ag = (uintptr_t)g, ab = (uintptr_t)buf;
  long long head = n, nvec = 0;
  if ((((ap ^ ag) | (ap ^ ab)) & 15) == 0) {
    head = (long long)(((16 - (ap & 15)) & 15) / 4);
    if (head > n) head = n;
    nvec = (n - head) / 4;
  }
  float4* __restrict__ p4 = reinterpret_cast<float4*>(p + head);
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
  float4* __restrict__ b4 = reinterpret_cast<float4*>(buf + head);
  for (long long i = tid; i < nvec; i += stride) {
    float4 pv = p4[i], bv = b4[i];
    const float4 gv = g4[i];
    sgd_update(pv.x, gv.x, bv.x, lr, momentum, weight_decay, grad_scale);
    sgd_update(pv.y, gv.y, bv.y, lr, momentum, weight_decay, grad_scale);
    sgd_update(pv.z, gv.z, bv.z, lr, momentum, weight_decay, grad_scale);
    sgd_update(pv.w, gv.w, bv.w, lr, momentum, weight_decay, grad_scale);
    b4[i] = bv;
    p4[i] = pv;
  }
  const long long tail0 = head + 4 * nvec, nscalar = head + (n - tail0);       // scalar elements: [0, head) and [tail0, n)
  for (long long i = tid; i < nscalar; i += stride) {
    const long long j = i < head ? i : tail0 + (i - head);
    float pj = p[j], bj = buf[j];
    sgd_update(pj, g[j], bj, lr, momentum, weight_decay, grad_scale);
    buf[j] = bj;
    p[j] = pj;
  }
}

__global__ void __launch_bounds__(kThreads) sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, long long n,
                                                       float lr, float momentum, float weight_decay, float grad_scale) {
  sgd_range(p, g, buf, n, lr, momentum, weight_decay, grad_scale);
}

// Graph-replayable form: hyper = {lr, momentum} in double (what the host form receives), narrowed once per thread exactly as the host
// form narrows its arguments; a scheduler changes lr by writing hyper[0].
__global__ void __launch_bounds__(kThreads) sgd_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                           long long n, const double* __restrict__ hyper, float weight_decay,
                                                           float grad_scale) {
  const float lr = (float)hyper[0], momentum = (float)hyper[1];
  sgd_range(p, g, buf, n, lr, momentum, weight_decay, grad_scale);
}

// Per-group learning rates over one arena range (FusedSGD with parameter groups: train.py --diff-lr).  The arena is a sequence of RUNS of
// equal group: seg_end[r] is the element offset one past run r (ascending, multiples of 4, the last one >= hi), seg_group[r] its group,
// group_lr[g] that group's learning rate as a double, all on the device, so the eager and the taped step are the same launch and a
// replayed tape follows a scheduler that writes group_lr.  Elements [lo, hi) of the arena, 16-byte accesses only (every offset is a
// multiple of 4 and the bases are 16-byte aligned), the same grid-stride walk as sgd_range: 20 bytes of traffic per element.
//
// The lookup stays off the memory path by being done per WAVE, not per lane.  A wave's 64 float4 are 256 consecutive elements; the run of
// their first element is a binary search whose every operand is wave-uniform (blockIdx, the loop counter, readfirstlane of the wave
// number), so the table is read with scalar loads through the scalar cache and the three 16-byte loads of the iteration, issued before
// it, are in flight meanwhile.  If that run also holds the wave's last element -- always, but for the few waves that straddle a slice
// boundary -- every lane takes the one rate.  A straddling wave searches per lane, but only between the runs of its first and last element.
// Any n_seg >= 1: nothing is staged, so nothing is capped.
__device__ __forceinline__ int sgd_run_of(const long long* __restrict__ seg_end, int first, int last, const long long e) {
  while (first < last) {                       // the smallest r in [first, last] with seg_end[r] > e; `last` when there is none
    const int mid = (first + last) >> 1;
    if (seg_end[mid] > e)
      last = mid;
    else
      first = mid + 1;
  }
  return first;
}

// The rate of run r, narrowed as sgd_dev_kernel narrows hyper[0].  A table that breaks its contract reads a wrong rate, never out of bounds.
__device__ __forceinline__ float sgd_group_lr(const int* __restrict__ seg_group, const double* __restrict__ group_lr, const int n_groups,
                                              const int r) {
  const int grp = seg_group[r];
  return (float)group_lr[grp < 0 ? 0 : (grp >= n_groups ? n_groups - 1 : grp)];
}

__global__ void __launch_bounds__(kThreads) sgd_groups_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                              const long long lo, const long long hi,
                                                              const long long* __restrict__ seg_end, const int* __restrict__ seg_group,
                                                              const int n_seg, const double* __restrict__ group_lr, const int n_groups,
                                                              const float momentum, const float weight_decay, const float grad_scale) {
  const long long v0 = lo >> 2, nvec = (hi - lo) >> 2, stride = (long long)gridDim.x * kThreads;
  float4* __restrict__ p4 = reinterpret_cast<float4*>(p) + v0;
  const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g) + v0;
  float4* __restrict__ b4 = reinterpret_cast<float4*>(buf) + v0;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (long long base = blockIdx.x * (long long)kThreads + wave * 64; base < nvec; base += stride) {        // wave-uniform
    const long long i = base + (threadIdx.x & 63);
    const bool live = i < nvec;
    float4 pv, bv, gv;
    if (live) {
      pv = p4[i];
      bv = b4[i];
      gv = g4[i];
    }
    const long long wlast = base + 63 < nvec ? base + 63 : nvec - 1;
    const int r0 = sgd_run_of(seg_end, 0, n_seg - 1, (v0 + base) << 2);
    float lr = sgd_group_lr(seg_group, group_lr, n_groups, r0);      // (wave-uniform: scalar loads again)
    if (seg_end[r0] <= ((v0 + wlast) << 2)) {                        // this wave straddles runs: each lane finds its own
      const int r1 = sgd_run_of(seg_end, r0, n_seg - 1, (v0 + wlast) << 2);
      const int r = sgd_run_of(seg_end, r0, r1, (v0 + (live ? i : base)) << 2);
      if (r != r0) lr = sgd_group_lr(seg_group, group_lr, n_groups, r);
    }
    if (live) {
      sgd_update(pv.x, gv.x, bv.x, lr, momentum, weight_decay, grad_scale);
      sgd_update(pv.y, gv.y, bv.y, lr, momentum, weight_decay, grad_scale);
      sgd_update(pv.z, gv.z, bv.z, lr, momentum, weight_decay, grad_scale);
      sgd_update(pv.w, gv.w, bv.w, lr, momentum, weight_decay, grad_scale);
      b4[i] = bv;
      p4[i] = pv;
    }
  }
}

}  // namespace dn

using namespace dn;

extern "C" {

int dn_adam_step(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2, double eps, double weight_decay,
                 int32_t step, double grad_scale, dn_stream_t stream) {
  DN_REQUIRE(p && g && m && v && n > 0 && step >= 1, DN_ERR_BAD_ARG, "dn_adam_step: bad argument");
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  const float step_size = (float)(lr / bc1);
  const float bc2_sqrt = (float)sqrt(bc2);
  DN_LAUNCH(adam_kernel, dim3(ew_blocks(n)), dim3(kThreads), 0, as_stream(stream), p, g, m, v, (long long)n, (float)beta1, (float)beta2, (float)eps,
                     (float)weight_decay, step_size, bc2_sqrt, (float)grad_scale);
  return check_launch("adam_kernel");
}

int dn_adam_step_dev(float* p, const float* g, float* m, float* v, int64_t n, const double* hyper, double eps, double weight_decay,
                     int32_t* step, float* derived, double grad_scale, dn_stream_t stream) {
  DN_REQUIRE(p && g && m && v && n > 0 && hyper && derived, DN_ERR_BAD_ARG, "dn_adam_step_dev: bad argument");
  hipStream_t s = as_stream(stream);
  if (step != nullptr) DN_LAUNCH(adam_tick_kernel, dim3(1), dim3(64), 0, s, step, hyper, derived);
  DN_LAUNCH(adam_dev_kernel, dim3(ew_blocks(n)), dim3(kThreads), 0, s, p, g, m, v, (long long)n, (float)eps, (float)weight_decay,
                     derived, (float)grad_scale);
  return check_launch("adam_dev_kernel");
}

int dn_adam_tick(const double* hyper, int32_t* step, float* derived, dn_stream_t stream) {
  DN_REQUIRE(hyper && step && derived, DN_ERR_BAD_ARG, "dn_adam_tick: bad argument");
  DN_LAUNCH(adam_tick_kernel, dim3(1), dim3(64), 0, as_stream(stream), step, hyper, derived);
  return check_launch("adam_tick_kernel");
}

int dn_sgd_step(float* p, const float* g, float* buf, int64_t n, double lr, double momentum, double weight_decay, double grad_scale,
                dn_stream_t stream) {
  DN_REQUIRE(p && g && buf && n > 0, DN_ERR_BAD_ARG, "dn_sgd_step: bad argument");
  DN_LAUNCH(sgd_kernel, dim3(ew_blocks((n + 3) / 4)), dim3(kThreads), 0, as_stream(stream), p, g, buf, (long long)n, (float)lr, (float)momentum,
                     (float)weight_decay, (float)grad_scale);
  return check_launch("sgd_kernel");
}

int dn_sgd_step_dev(float* p, const float* g, float* buf, int64_t n, const double* hyper, double weight_decay, double grad_scale,
                    dn_stream_t stream) {
  DN_REQUIRE(p && g && buf && n > 0 && hyper, DN_ERR_BAD_ARG, "dn_sgd_step_dev: bad argument");
  DN_LAUNCH(sgd_dev_kernel, dim3(ew_blocks((n + 3) / 4)), dim3(kThreads), 0, as_stream(stream), p, g, buf, (long long)n, hyper,
                     (float)weight_decay, (float)grad_scale);
  return check_launch("sgd_dev_kernel");
}

int dn_sgd_step_groups(float* p, const float* g, float* buf, int64_t lo, int64_t hi, const int64_t* seg_end, const int32_t* seg_group,
                       int32_t n_seg, const double* group_lr, int32_t n_groups, double momentum, double weight_decay, double grad_scale,
                       dn_stream_t stream) {
  const uintptr_t bases = (uintptr_t)p | (uintptr_t)g | (uintptr_t)buf;
  DN_REQUIRE(p && g && buf && seg_end && seg_group && group_lr && lo >= 0 && hi > lo && n_seg >= 1 && n_groups >= 1 &&
                 (bases & 15) == 0 && ((lo | hi) & 3) == 0,
             DN_ERR_BAD_ARG, "dn_sgd_step_groups: bad argument");
  DN_LAUNCH(sgd_groups_kernel, dim3(ew_blocks((hi - lo) / 4)), dim3(kThreads), 0, as_stream(stream), p, g, buf, (long long)lo, (long long)hi,
            reinterpret_cast<const long long*>(seg_end), reinterpret_cast<const int*>(seg_group), (int)n_seg, group_lr, (int)n_groups,
            (float)momentum, (float)weight_decay, (float)grad_scale);
  return check_launch("sgd_groups_kernel");
}

}  // extern "C"
