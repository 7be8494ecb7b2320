// Which kernel a conv call runs, and the conv entry points of the ABI.  Host code only: every kernel family lives in a file of its
// own and exports an *_eligible and a launch_* through dn_internal.h.
//
//   forward / input gradient / conv-transpose : kConvFamilies, first eligible row (conv_route); run_conv launches it, the weight re-lay
//                                               and the host queries of dn_plan.hip read its columns
//   weight gradient                           : kWgradFamilies (sizing and launch read the same rows), then the leading-pieces split,
//                                               the tap windows and the tiled kernel (dn_tiled_wgrad.hip)
#include <stdlib.h>

#include "dn_internal.h"

namespace dn {

// The forward / input-gradient / conv-transpose kernel families in priority order; the tiled kernels, last, take every plan.  conv_route
// returns the first eligible row: run_conv launches it, the weight re-lay follows its layout, and the host queries of dn_plan.hip -- on
// whose answers the engine allocates recip_out, skips dn_bn_finalize and takes sums for finished -- read its columns.  Which template
// instance a row runs (tile shape, Winograd variant) is its launch's business.  A new family adds one row here.
template <auto Launch> static int plan_only(const dn_conv_desc*, IgemmParams& p, hipStream_t s) { return Launch(p, s); }
template <auto Launch> static int with_desc(const dn_conv_desc* d, IgemmParams& p, hipStream_t s) { return Launch(d, p, s); }
static bool heads_off() { return knobs().no_direct; }
// Split-K bytes of every row but Winograd's: the three-piece tiled kernel's.  Only the tiled row splits; for the others it is an upper
// bound that no launch of the row uses, kept because that is what callers have always been told.
constexpr auto x3_upper = conv_x3_splitk_workspace_upper_bytes;
static const ConvFamily kConvFamilies[] = {
    {"head_fwd", head_fwd_eligible, heads_off, plan_only<launch_head_fwd>, nullptr, x3_upper, head_fwd_fuses_reciprocal},
    {"head_dgrad", head_dgrad_eligible, heads_off, plan_only<launch_head_dgrad>, nullptr, x3_upper},
    {"winograd", wino_eligible, nullptr, plan_only<launch_wino_conv>, wino_layout,
     [](const IgemmParams& p) { return wino_layout(p) == 3 ? wino_splitk_workspace_bytes(p) : (size_t)0; }, nullptr,
     [](const dn_conv_desc* d) {
       const dn_result& r = d->out[0];
       return d->kind == DN_CONV_DGRAD && d->n_out == 1 && !r.accumulate && (r.C & 3) == 0 && r.stride_w == r.C &&
              r.stride_h == (int64_t)d->OW * r.C && r.stride_n == (int64_t)d->OH * d->OW * r.C && d->bias == nullptr && d->act == DN_ACT_NONE;
     },
     [](IgemmParams& p) { wino_prepare(p); return wino_folds_bn_finalize(p); }, [](IgemmParams& p) { wino_prepare(p); return wino_folds_bn_sums(p); }},
    {"stem3", stem3_conv_eligible, nullptr, plan_only<launch_stem3_conv>, nullptr, x3_upper},
    {"stemk", stemk_conv_eligible, nullptr, with_desc<launch_stemk_conv>, nullptr, x3_upper},
    {"stem", stem_eligible, nullptr, plan_only<launch_stem>, nullptr, x3_upper},
    {"lds3", lds3_conv_eligible, nullptr, with_desc<launch_lds3_conv>, nullptr, x3_upper},
    {"lds3k", lds3k_conv_eligible, nullptr, with_desc<launch_lds3k_conv>, nullptr, x3_upper},
    {"thin", thin_conv_eligible, nullptr, plan_only<launch_thin_conv>, nullptr, x3_upper},
    {"tiled", [](const dn_conv_desc*, const IgemmParams&) { return true; }, nullptr, plan_only<launch_tiled_conv>, nullptr, x3_upper},
};

const ConvFamily* conv_route(const dn_conv_desc* d, const IgemmParams& p) {
  const ConvFamily* f = kConvFamilies;
  while (!f->eligible(d, p) || (f->switched_off && f->switched_off())) ++f;
  return f;
}

static int run_conv(const dn_conv_desc* d, int expect_kind, dn_stream_t stream) {
  DN_REQUIRE(d != nullptr && d->kind == expect_kind, DN_ERR_BAD_ARG, "descriptor kind mismatch (want %d)", expect_kind);
  IgemmParams p;
  int rc = build_plan(d, false, &p);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(p.w != nullptr, DN_ERR_BAD_ARG, "w_packed is null");
  for (int i = 0; i < p.n_in; ++i) DN_REQUIRE(p.in[i].p != nullptr, DN_ERR_BAD_ARG, "operand %d has no data", i);
  for (int i = 0; i < p.n_out; ++i) {
    const dn_result& o = d->out[i];
    DN_REQUIRE(o.stride_h == (int64_t)d->OW * o.stride_w && o.stride_n == (int64_t)d->OH * o.stride_h, DN_ERR_UNSUPPORTED,
               "result %d must be pixel-dense (NHWC with a channel stride)", i);
  }
  return conv_route(d, p)->launch(d, p, as_stream(stream));
}

}  // namespace dn

using namespace dn;

// A concatenated input whose LAST piece is a 1-channel map (the upsampled disparity of the iconv layers: 64 + 128 + 1, 64 + 256 + 1):
// the 1-channel piece is what keeps the layer off the Winograd weight-gradient kernel (operands in multiples of 64).  Split the
// gradient instead: Winograd for the pieces in front (rows of dw written with the full layer's channel stride), the tiled kernel for
// the one trailing channel (9 columns of dw).  iconv2 at 32 images: 0.272 -> 0.15 ms; config 4's 321 -> 64 @120x160: 1.25 -> 0.5 ms.
static bool wgrad_split_plans(const dn_conv_desc* fwd, dn_conv_desc* d1, dn_conv_desc* d2, IgemmParams* p1, IgemmParams* p2, size_t* w1,
                              size_t* w2) {
  if (fwd->kind != DN_CONV_FWD || fwd->n_in < 2 || fwd->in[fwd->n_in - 1].C != 1) return false;
  *d1 = *fwd;
  d1->n_in = fwd->n_in - 1;
  *d2 = *fwd;
  d2->n_in = 1;
  d2->in[0] = fwd->in[fwd->n_in - 1];
  if (build_plan(d1, true, p1) != DN_OK || build_plan(d2, true, p2) != DN_OK) return false;
  int cin_total = 0;
  for (int i = 0; i < fwd->n_in; ++i) cin_total += fwd->in[i].C;
  if (wino_wgrad_eligible(d1, *p1)) {
    p1->dw_cin_total = cin_total;
    *w1 = (wino_wgrad_workspace_bytes(*p1) + 255) / 256 * 256;
  } else {
    // (round 4 measured the pieces in front on the three-piece tiled kernel: SLOWER -- iconv1 97 -> 32 @64x208 0.375 -> 0.508 ms, a 32-wide
    //  n tile is bound by its staging; the switch that kept that path alive was removed in round 5)
    return false;
  }
  p2->in[0].ch_off = cin_total - 1;              // (packed_to_framework: the column block of this channel in the full weight tensor)
  p2->D1 = cin_total;
  choose_splits(p2);
  *w2 = generic_wgrad_workspace_bytes(*p2);
  return true;
}

// Kernels of more than 32 taps (the 7x7 / stride-2 first layers of ResNet-50 and PoseExpNet: reference models/Disp_res_50.py:65,141,
// models/PoseExpNet.py:28): the scheduled weight-gradient kernels carry one validity bit per tap in a 32-bit word, so such layers fell to
// the unscheduled kernel (1.30 ms at 18 TFLOP/s in config 4, 0.57 ms in config 3).  The taps are independent columns of dW, so the
// gradient is taken as two launches over tap WINDOWS of <= 32 taps each, every one with the full plan's operands and its own rows of the
// tap tables; the split sum of each window writes only its own (r, s) entries of dw.
static int tap_windows(const IgemmParams& p) {
  const int nt = p.ph[0].ntaps;
  if (nt <= 32 || p.reflect || p.nphases != 1 || knobs().no_tap_windows) return 1;
  return (nt + 31) / 32;
}

static void tap_window_plan(const IgemmParams& full, int w, int nw, IgemmParams* q) {
  *q = full;
  const int nt = full.ph[0].ntaps, per = (nt + nw - 1) / nw;
  const int t0 = w * per, t1 = t0 + per < nt ? t0 + per : nt;
  for (int t = t0; t < t1; ++t) {
    q->tdy[t - t0] = full.tdy[full.ph[0].tap0 + t];
    q->tdx[t - t0] = full.tdx[full.ph[0].tap0 + t];
    q->tr[t - t0] = full.tr[full.ph[0].tap0 + t];
    q->ts[t - t0] = full.ts[full.ph[0].tap0 + t];
  }
  q->ph[0].tap0 = 0;
  q->ph[0].ntaps = t1 - t0;
  int nch = 0;
  for (int i = 0; i < q->n_in; ++i) nch += (q->ph[0].ntaps * q->in[i].C + kChunk - 1) / kChunk;
  q->ph[0].nchunks = nch;
  q->uni32 = 1;
  q->wg_uniform = 1;
  for (int i = 0; i < q->n_in; ++i) {
    const KOperand& o = q->in[i];
    if (!o.small) q->uni32 = 0;
    if (!o.small || (!o.vec && o.scale != nullptr) || o.C >= 32768) q->wg_uniform = 0;
  }
}

// The weight-gradient kernel families in front of the tiled kernel, in priority order.  dn_conv_wgrad_workspace_bytes takes the
// largest workspace_bytes of the eligible rows; dn_conv2d_wgrad launches the first eligible row whose workspace fits (a caller
// that brought less falls through to the next row, in the end to the tiled kernel).  A new family adds one row here.
struct WgradFamily {
  const char* name;
  bool (*eligible)(const dn_conv_desc* fwd, const IgemmParams& p);
  size_t (*workspace_bytes)(const dn_conv_desc* fwd, const IgemmParams& p);
  bool dy_aligned16;            // the kernel reads dy as float4
  bool (*switched_off)();       // launch-time switch (the sizing ignores it), or nullptr
  int (*launch)(const dn_conv_desc* fwd, IgemmParams& p, float* dw, hipStream_t s);
};
static const WgradFamily kWgradFamilies[] = {
    {"head", head_wgrad_eligible, [](const dn_conv_desc*, const IgemmParams& p) { return head_wgrad_workspace_bytes(p); }, false,
     [] { return knobs().no_direct; },       // (the head has one operand; its slabs are an argument of their own)
     [](const dn_conv_desc*, IgemmParams& p, float* dw, hipStream_t s) { return launch_head_wgrad(p, dw, p.ws, s); }},
    {"winograd", wino_wgrad_eligible, [](const dn_conv_desc*, const IgemmParams& p) { return wino_wgrad_workspace_bytes(p); }, false, nullptr,
     [](const dn_conv_desc*, IgemmParams& p, float* dw, hipStream_t s) { return launch_wino_wgrad(p, dw, s); }},
    {"lds3", lds3_wgrad_eligible, [](const dn_conv_desc*, const IgemmParams& p) { return lds3_wgrad_workspace_bytes(p); }, true, nullptr,
     launch_lds3_wgrad},
    {"lds3k", lds3k_wgrad_eligible, [](const dn_conv_desc*, const IgemmParams& p) { return lds3k_wgrad_workspace_bytes(p); }, true, nullptr,
     launch_lds3k_wgrad},
    // 7x7 / stride-2 first layers on NCHW images (dn_stemk.hip)
    {"stemk", stemk_wgrad_eligible, stemk_wgrad_workspace_bytes, true, nullptr, launch_stemk_wgrad},
    {"thin", thin_wgrad_eligible, [](const dn_conv_desc*, const IgemmParams& p) { return thin_wgrad_workspace_bytes(p); }, false, nullptr,
     [](const dn_conv_desc*, IgemmParams& p, float* dw, hipStream_t s) { return launch_thin_wgrad(p, dw, s); }},
};

extern "C" {

int64_t dn_pack_entry_bytes(void) { return (int64_t)sizeof(PackEntry); }

int dn_pack_entry_fill(const dn_conv_desc* d, const float* w, float* w_packed, void* entry_host) {
  DN_REQUIRE(d && w && w_packed && entry_host, DN_ERR_BAD_ARG, "dn_pack_entry_fill: null pointer");
  PackEntry* e = reinterpret_cast<PackEntry*>(entry_host);
  int rc = build_plan(d, false, &e->p);
  if (rc != DN_OK) return rc;
  e->w = w;
  e->wp = w_packed;
  const ConvFamily* f = conv_route(d, e->p);
  e->wino = f->weight_layout ? f->weight_layout(e->p) : 0;
  if (e->wino) {
    e->total = wino_packed_elems(e->p);
    e->NS = ((e->p.Ntot + 63) / 64 * 64) / 32;
  } else {
    e->total = direct_packed_elems(e->p);
    e->NS = 0;
  }
  return e->wino;
}

int dn_pack_many(const void* entries_dev, int32_t n_direct, int32_t n_wino, int32_t n_wino16, int32_t n_wino_x3, dn_stream_t stream) {
  DN_REQUIRE(entries_dev && n_direct >= 0 && n_wino >= 0 && n_wino16 >= 0 && n_wino_x3 >= 0, DN_ERR_BAD_ARG, "dn_pack_many: bad argument");
  const PackEntry* tab = reinterpret_cast<const PackEntry*>(entries_dev);
  hipStream_t s = as_stream(stream);
  if (n_direct > 0) {
    int rc = launch_direct_pack_many(tab, n_direct, s);
    if (rc != DN_OK) return rc;
  }
  if (n_wino > 0) {
    int rc = launch_wino_pack_many(tab, n_direct, n_wino, s);
    if (rc != DN_OK) return rc;
  }
  if (n_wino16 > 0) {
    int rc = launch_wino_pack16_many(tab, n_direct + n_wino, n_wino16, 1, s);
    if (rc != DN_OK) return rc;
  }
  if (n_wino_x3 > 0) return launch_wino_pack16_many(tab, n_direct + n_wino + n_wino16, n_wino_x3, 3, s);
  return DN_OK;
}

int dn_conv_pack_weights(const dn_conv_desc* d, const float* w, float* w_packed, dn_stream_t stream) {
  IgemmParams p;
  int rc = build_plan(d, false, &p);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(w != nullptr && w_packed != nullptr, DN_ERR_BAD_ARG, "null weight pointer");
  const ConvFamily* f = conv_route(d, p);
  if (const int wl = f->weight_layout ? f->weight_layout(p) : 0)
    return wl == 1 ? launch_wino_pack(p, w, w_packed, as_stream(stream)) : launch_wino_pack16(p, w, w_packed, wl == 3 ? 3 : 1, as_stream(stream));
  return launch_direct_pack(p, w, w_packed, as_stream(stream));
}

int dn_conv2d_fwd(const dn_conv_desc* d, dn_stream_t stream) { return run_conv(d, DN_CONV_FWD, stream); }
int dn_conv2d_dgrad(const dn_conv_desc* d, dn_stream_t stream) { return run_conv(d, DN_CONV_DGRAD, stream); }
int dn_convT2d_fwd(const dn_conv_desc* d, dn_stream_t stream) { return run_conv(d, DN_CONVT_FWD, stream); }
int dn_convT2d_dgrad(const dn_conv_desc* d, dn_stream_t stream) { return run_conv(d, DN_CONVT_DGRAD, stream); }

size_t dn_conv_wgrad_workspace_bytes(const dn_conv_desc* fwd) {
  IgemmParams p;
  if (build_plan(fwd, true, &p) != DN_OK) return 0;
  choose_splits(&p);
  size_t need = generic_wgrad_workspace_bytes(p);
  for (const WgradFamily& f : kWgradFamilies)
    if (f.eligible(fwd, p) && f.workspace_bytes(fwd, p) > need) need = f.workspace_bytes(fwd, p);
  {
    dn_conv_desc d1, d2;
    IgemmParams p1, p2;
    size_t w1 = 0, w2 = 0;
    if (wgrad_split_plans(fwd, &d1, &d2, &p1, &p2, &w1, &w2) && w1 + w2 > need) need = w1 + w2;
  }
  const int nw = tap_windows(p);
  for (int w = 0; w < nw && nw > 1; ++w) {
    IgemmParams q;
    tap_window_plan(p, w, nw, &q);
    choose_splits(&q);
    if (generic_wgrad_workspace_bytes(q) > need) need = generic_wgrad_workspace_bytes(q);
  }
  return need;
}

int dn_conv2d_wgrad(const dn_conv_desc* fwd, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                    dn_stream_t stream) {
  IgemmParams p;
  int rc = build_plan(fwd, true, &p);
  if (rc != DN_OK) return rc;
  DN_REQUIRE(dy != nullptr && dw != nullptr && workspace != nullptr, DN_ERR_BAD_ARG, "null pointer");
  const hipStream_t s = as_stream(stream);
  for (const WgradFamily& f : kWgradFamilies) {
    if (!f.eligible(fwd, p) || (f.switched_off && f.switched_off()) || workspace_bytes < f.workspace_bytes(fwd, p)) continue;
    if (f.dy_aligned16 && (reinterpret_cast<uintptr_t>(dy) & 15) != 0) continue;
    for (int i = 0; i < p.n_in; ++i) DN_REQUIRE(p.in[i].p != nullptr, DN_ERR_BAD_ARG, "operand %d has no data", i);
    p.g = dy;
    p.ws = reinterpret_cast<float*>(workspace);
    return f.launch(fwd, p, dw, s);
  }
  {
    dn_conv_desc d1, d2;
    IgemmParams p1, p2;
    size_t w1 = 0, w2 = 0;
    if (wgrad_split_plans(fwd, &d1, &d2, &p1, &p2, &w1, &w2) && workspace_bytes >= w1 + w2) {
      for (int i = 0; i < fwd->n_in; ++i) DN_REQUIRE(fwd->in[i].data != nullptr, DN_ERR_BAD_ARG, "operand %d has no data", i);
      if (wino_wgrad_eligible(&d1, p1)) {
        p1.g = dy;
        p1.ws = reinterpret_cast<float*>(workspace);
        rc = launch_wino_wgrad(p1, dw, s);
      } else {
        rc = generic_wgrad(&d1, p1, dy, dw, workspace, w1, s);
      }
      if (rc != DN_OK) return rc;
      return generic_wgrad(&d2, p2, dy, dw, reinterpret_cast<char*>(workspace) + w1, w2, s);
    }
  }
  if (const int nw = tap_windows(p); nw > 1 && fwd->kind == DN_CONV_FWD) {
    for (int w = 0; w < nw; ++w) {
      IgemmParams q;
      tap_window_plan(p, w, nw, &q);
      rc = generic_wgrad(fwd, q, dy, dw, workspace, workspace_bytes, s);
      if (rc != DN_OK) return rc;
    }
    return DN_OK;
  }
  return generic_wgrad(fwd, p, dy, dw, workspace, workspace_bytes, s);
}

}  // extern "C"
