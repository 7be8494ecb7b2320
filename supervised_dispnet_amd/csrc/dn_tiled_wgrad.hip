// The tiled weight gradient on the fp32 matrix core -- what every layer no row of kWgradFamilies (dn_conv.hip) takes runs -- with its
// fixed-order split sum, and the direct (implicit-GEMM) weight re-lay, which shares packed_to_framework with that sum.
#include "dn_igemm.h"

namespace dn {

// ----------------------------------------------------------------------------------------------- weight gradient
// ws[split][n][k] = sum over the split's pixels of G[pixel][n] * A[pixel][k].  Tile: BNW (n) x 128 (k), 32 pixels per step.
// ALLVEC (every gathered operand and G float4-addressable with int32 offsets): straight-line staging, see igemm_conv_kernel.
template <int BNW, int WNn, int WKk, bool ALLVEC>
__global__ void __launch_bounds__(256, 2) igemm_wgrad_kernel(const IgemmParams p) {
  constexpr int BKW = 128;
  constexpr int WAVES_K = BKW / WKk;
  constexpr int NI = WNn / 32, KI = WKk / 32;
  constexpr int GR = BNW / 32;  // float4 groups per thread for the G tile
  static_assert((BNW / WNn) * WAVES_K == 4, "4 waves per block");
  extern __shared__ __align__(16) float smem[];
  float* Gs = smem;                                        // [2][32][BNW]
  float* Xs = smem + 2 * 32 * BNW;                         // [2][32][BKW]
  int* taps = reinterpret_cast<int*>(Xs + 2 * 32 * BKW);   // [kMaxTaps]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave / WAVES_K, wk = wave % WAVES_K;
  const int kt = blockIdx.x, n0 = blockIdx.y * BNW;
  const KPhase ph = p.ph[0];
  const int ntaps = ph.ntaps, nchunks = ph.nchunks, Kp = nchunks * kChunk;
  const int m_begin = blockIdx.z * p.m_per_split;
  const int m_end = min(p.M, m_begin + p.m_per_split);

  if (tid < ntaps) taps[tid] = ((int)p.tdy[tid] & 0xffff) | ((int)p.tdx[tid] << 16);
  __syncthreads();

  const int g = tid & 7, r = tid >> 3;  // staging: row r of the 32-pixel step, 4-float group g
  // fixed per-thread K selections for the 4 chunks of this k tile
  int q_s[4], q_j[4], q_c[4], q_kl[4], q_dy[4], q_dx[4];
  bool q_live[4], q_kvalid[4];
  f32x4 xsc[4], xsh[4];
  float q_floor[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    int kc = kt * 4 + q;
    q_live[q] = kc < nchunks;
    int kcl = 0;
    q_s[q] = q_live[q] ? select_operand(p, ntaps, kc, &kcl) : 0;
    q_kl[q] = kcl * kChunk + g * 4;
    const KOperand& S = p.in[q_s[q]];
    q_j[q] = q_kl[q] / S.C;
    q_c[q] = q_kl[q] - q_j[q] * S.C;
    q_kvalid[q] = q_live[q] && q_j[q] < ntaps;
    const int t = taps[q_kvalid[q] ? q_j[q] : 0];
    q_dy[q] = (int)(short)(t & 0xffff);
    q_dx[q] = t >> 16;
    if constexpr (ALLVEC) {
      const bool has_aff = S.scale != nullptr;
      const f32x4 l1 = *reinterpret_cast<const f32x4*>((has_aff ? S.scale : S.p) + q_c[q]);
      const f32x4 l2 = *reinterpret_cast<const f32x4*>((has_aff ? S.shift : S.p) + q_c[q]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        xsc[q][e] = has_aff ? l1[e] : 1.f;
        xsh[q][e] = has_aff ? l2[e] : 0.f;
      }
      q_floor[q] = has_aff ? 0.f : -__builtin_huge_valf();
    }
  }
  const bool gvec = (p.Ntot % 4 == 0);

  f32x16 acc[NI][KI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < KI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  f32x4 gv[GR];
  AGroup xv[4];
  bool xaff[4];

  auto issue_loads = [&](int mbase) {
    const int m = mbase + r;
    const bool rowvalid = m < m_end;
    if constexpr (ALLVEC) {
      unsigned gx, gy;
      const unsigned mm = rowvalid ? (unsigned)m : 0u;
      const unsigned t = fastdiv_dev(mm, (unsigned)p.GW, p.mGW, &gx);
      const int n = (int)fastdiv_dev(t, (unsigned)p.GH, p.mGH, &gy);
      const int by = (int)gy * p.sy, bx = (int)gx * p.sx;
      const int grow = (int)mm * p.Ntot + n0 + g * 4;
#pragma unroll
      for (int i = 0; i < GR; ++i) {
        const bool ok = rowvalid && (n0 + g * 4 + 32 * i) < p.Ntot;
        const f32x4 v = *reinterpret_cast<const f32x4*>(p.g + (ok ? grow + 32 * i : 0));
#pragma unroll
        for (int e = 0; e < 4; ++e) gv[i][e] = ok ? v[e] : 0.f;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const KOperand& S = p.in[q_s[q]];
        int iy = by + q_dy[q], ix = bx + q_dx[q];
        if (p.reflect) {
          iy = reflect_idx(iy, p.IH);
          ix = reflect_idx(ix, p.IW);
        }
        const bool ok = rowvalid && q_kvalid[q] && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW;
        int off = n * (int)S.sn + (iy >> S.up) * (int)S.sh + (ix >> S.up) * (int)S.sw + q_c[q];
        off = ok ? off : 0;
        xv[q].v = *reinterpret_cast<const f32x4*>(S.p + off);
        xv[q].ok = ok;
      }
    } else {
      int n = 0, by = 0, bx = 0;
      if (rowvalid) {
        int gx = m % p.GW, t = m / p.GW;
        int gy = t % p.GH;
        n = t / p.GH;
        by = gy * p.sy;
        bx = gx * p.sx;
      }
#pragma unroll
      for (int i = 0; i < GR; ++i) {
        const int col = n0 + g * 4 + 32 * i;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (rowvalid) {
          const float* gp = p.g + (long long)m * p.Ntot + col;
          if (gvec) {
            if (col < p.Ntot) v = *reinterpret_cast<const f32x4*>(gp);
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (col + e < p.Ntot) v[e] = gp[e];
          }
        }
        gv[i] = v;
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        xaff[q] = false;
        if (q_live[q]) {
          const KOperand& S = p.in[q_s[q]];
          if (S.vec && S.scale != nullptr && q_j[q] < ntaps) {
            xsc[q] = *reinterpret_cast<const f32x4*>(S.scale + q_c[q]);
            xsh[q] = *reinterpret_cast<const f32x4*>(S.shift + q_c[q]);
            xaff[q] = true;
          }
          xv[q] = gather4(S, q_kl[q], ntaps, taps, n, by, bx, rowvalid, p.IH, p.IW, q_j[q], q_c[q], p.reflect);
        } else {
          xv[q].v = f32x4{0.f, 0.f, 0.f, 0.f};
          xv[q].ok = false;
        }
      }
    }
  };

  auto store_stage = [&](int buf) {
    float* gs = Gs + buf * 32 * BNW + r * BNW + g * 4;
#pragma unroll
    for (int i = 0; i < GR; ++i) *reinterpret_cast<f32x4*>(gs + 32 * i) = gv[i];
    float* xs = Xs + buf * 32 * BKW + r * BKW + g * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 v = xv[q].v;
      if constexpr (ALLVEC) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float t = fmaxf(q_floor[q], fmaf(v[e], xsc[q][e], xsh[q][e]));
          v[e] = xv[q].ok ? t : 0.f;
        }
      } else {
        if (xaff[q]) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(0.f, v[e] * xsc[q][e] + xsh[q][e]);
        }
        if (!xv[q].ok) v = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      *reinterpret_cast<f32x4*>(xs + 32 * q) = v;
    }
  };

  const int nsteps = (m_end > m_begin) ? (m_end - m_begin + 31) / 32 : 0;
  if (nsteps > 0) {
    issue_loads(m_begin);
    store_stage(0);
  }
  __syncthreads();
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    const bool more = st + 1 < nsteps;
    if constexpr (ALLVEC) {
      issue_loads(m_begin + (more ? st + 1 : st) * 32);
      __builtin_amdgcn_sched_barrier(0);
    } else {
      if (more) issue_loads(m_begin + (st + 1) * 32);
    }
    const float* Gb = Gs + buf * 32 * BNW + (lane >> 5) * BNW + wn * WNn + (lane & 31);
    const float* Xb = Xs + buf * 32 * BKW + (lane >> 5) * BKW + wk * WKk + (lane & 31);
#pragma unroll
    for (int s2 = 0; s2 < 16; ++s2) {
      float a[NI], b[KI];
#pragma unroll
      for (int i = 0; i < NI; ++i) a[i] = Gb[s2 * 2 * BNW + i * 32];
#pragma unroll
      for (int j = 0; j < KI; ++j) b[j] = Xb[s2 * 2 * BKW + j * 32];
#pragma unroll
      for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < KI; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    if constexpr (ALLVEC) {
      __builtin_amdgcn_sched_barrier(0);
      store_stage(buf ^ 1);
    } else {
      if (more) store_stage(buf ^ 1);
    }
    __syncthreads();
  }

  float* ws = p.ws + (long long)blockIdx.z * p.Npad * Kp;
#pragma unroll
  for (int j = 0; j < KI; ++j) {
    const int k = kt * BKW + wk * WKk + j * 32 + (lane & 31);
    if (k >= Kp) continue;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + wn * WNn + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        ws[(long long)n * Kp + k] = acc[i][j][reg];
      }
  }
}

// ------------------------------------------------------------------------------------ weight gradient, fast path
// The 4 K chunks of this block's k tile are LOOP-INVARIANT (the loop runs over pixels), so everything about them is decided
// once: a chunk of a float4-addressable operand (any C % 4 == 0) gives each thread one (tap, channel) for its K group -- kept
// as per-thread registers, block-uniform when C % 32 == 0; a chunk of a scalar operand (the 1-channel disparity piece, the
// 3-channel NCHW image) gives it four (tap, channel) pairs and is gathered pixel-major so the loads coalesce.  Hand-scheduled
// like igemm_conv_u32_kernel: the next 32-pixel step's loads and address arithmetic are dealt under the first MFMAs of the
// current step, the LDS fragment reads one pixel pair ahead of their MFMAs, the store stage under the last MFMAs.  The chunk
// kind tests are block-uniform branches inside the slots; they do not disturb the slot order.
template <int BNW, int WNn, int WKk, bool AFF>
__global__ void __launch_bounds__(256, 2) igemm_wgrad_u32_kernel(const IgemmParams p) {
  constexpr int BKW = 128;
  constexpr int WAVES_K = BKW / WKk;
  constexpr int NI = WNn / 32, KI = WKk / 32;
  constexpr int GR = BNW / 32;  // float4 groups per thread for the G tile
  static_assert((BNW / WNn) * WAVES_K == 4, "4 waves per block");
  extern __shared__ __align__(16) float smem[];
  float* Gs = smem;                                        // [2][32][BNW]
  float* Xs = smem + 2 * 32 * BNW;                         // [2][32][BKW]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave / WAVES_K, wk = wave % WAVES_K;
  const KPhase ph = p.ph[0];
  const int ntaps = ph.ntaps, nchunks = ph.nchunks, Kp = nchunks * kChunk;
  // XCD-aware order (see igemm_conv_u32_kernel): the k tiles and n tiles of ONE pixel split are consecutive logical tiles
  // on one XCD, so they run side by side on one L2 and the split's G / X pixels come over the fabric once, not once per tile.
  const int KT = (nchunks + 3) / 4, NTn = p.Npad / BNW;
  const int total = KT * NTn * p.splits;
  const int per = (total + 7) >> 3;
  const int lq = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
  if ((int)(blockIdx.x >> 3) >= per || lq >= total) return;
  const int kt = lq % KT, n0 = ((lq / KT) % NTn) * BNW, split = lq / (KT * NTn);
  const int m_begin = split * p.m_per_split;
  const int m_end = min(p.M, m_begin + p.m_per_split);
  const int g = tid & 7, r = tid >> 3;      // float4 staging: row r of the 32-pixel step, K group g
  const int g2 = tid >> 5, r2 = tid & 31;   // scalar-chunk staging: pixel-major (lanes = consecutive pixels), K group g2

  // chunk descriptors (block-uniform part in SGPRs, per-thread tap / channel in VGPRs)
  const char* qbase[4];
  int qsn[4], qsh[4], qsw[4], qsc[4], qup[4];
  bool qvec[4], qscal[4];
  int qtap[4];            // vec chunk: this thread's (dy | dx << 16), or 0x80008000 when its K group is past the last tap
  unsigned qoffB[4];      // vec chunk: this thread's channel byte offset
  int qst[4][4];          // scalar chunk: per element (dy & 0xff) | (dx & 0xff) << 8 | channel << 16, or -1 when dead
  f32x4 xsc[4], xsh[4];
  float qfloor[4];
  bool any_scalar = false;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int kc = kt * 4 + q;
    int kcl = 0;
    const bool live = kc < nchunks;
    const int s = live ? select_operand(p, ntaps, kc, &kcl) : 0;
    const KOperand& S = p.in[s];
    qbase[q] = reinterpret_cast<const char*>(S.p);
    qsn[q] = __builtin_amdgcn_readfirstlane((int)S.sn);
    qsh[q] = __builtin_amdgcn_readfirstlane((int)S.sh);
    qsw[q] = __builtin_amdgcn_readfirstlane((int)S.sw);
    qsc[q] = __builtin_amdgcn_readfirstlane((int)S.sc);
    qup[q] = __builtin_amdgcn_readfirstlane(S.up);
    qvec[q] = live && S.vec;
    qscal[q] = live && !S.vec;
    any_scalar = any_scalar || qscal[q];
    {
      unsigned c;
      const int j = (int)fastdiv_dev((unsigned)(kcl * kChunk + g * 4), (unsigned)S.C, S.mC, &c);
      const bool ok = qvec[q] && j < ntaps;
      const int jj = ok ? j : 0;
      qtap[q] = ok ? (((int)p.tdy[jj] & 0xffff) | ((int)p.tdx[jj] << 16)) : (int)0x80008000;
      qoffB[q] = ok ? c * 4u : 0u;
      if constexpr (AFF) {
        const bool has_aff = ok && S.scale != nullptr;
        const f32x4 l1 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(has_aff ? S.scale : S.p) + qoffB[q]);
        const f32x4 l2 = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(has_aff ? S.shift : S.p) + qoffB[q]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          xsc[q][e] = has_aff ? l1[e] : 1.f;
          xsh[q][e] = has_aff ? l2[e] : 0.f;
        }
        qfloor[q] = has_aff ? 0.f : -__builtin_huge_valf();
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      unsigned c;
      const int j = (int)fastdiv_dev((unsigned)(kcl * kChunk + g2 * 4 + e), (unsigned)S.C, S.mC, &c);
      const bool ok = qscal[q] && j < ntaps;
      const int jj = ok ? j : 0;
      qst[q][e] = ok ? (((int)p.tdy[jj] & 0xff) | (((int)p.tdx[jj] & 0xff) << 8) | ((int)c << 16)) : -1;
    }
  }

  f32x16 acc[NI][KI];
#pragma unroll
  for (int i = 0; i < NI; ++i)
#pragma unroll
    for (int j = 0; j < KI; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const char* gbase = reinterpret_cast<const char*>(p.g);
  f32x4 gv[GR], xv[4];
  bool xok[4], rowvalid = false, rowvalid2 = false;
  int pn = 0, pby = 0, pbx = 0, pn2 = 0, pby2 = 0, pbx2 = 0;
  unsigned goffB = 0;

  auto decode_pixel = [&](int mbase) {
    const int m = mbase + r;
    rowvalid = m < m_end;
    const unsigned mm = rowvalid ? (unsigned)m : 0u;
    unsigned gx, gy;
    const unsigned t = fastdiv_dev(mm, (unsigned)p.GW, p.mGW, &gx);
    pn = (int)fastdiv_dev(t, (unsigned)p.GH, p.mGH, &gy);
    pby = (int)gy * p.sy;
    pbx = (int)gx * p.sx;
    goffB = (mm * (unsigned)p.Ntot + (unsigned)(n0 + g * 4)) * 4u;
    if (any_scalar) {
      const int m2 = mbase + r2;
      rowvalid2 = m2 < m_end;
      const unsigned t2 = fastdiv_dev(rowvalid2 ? (unsigned)m2 : 0u, (unsigned)p.GW, p.mGW, &gx);
      pn2 = (int)fastdiv_dev(t2, (unsigned)p.GH, p.mGH, &gy);
      pby2 = (int)gy * p.sy;
      pbx2 = (int)gx * p.sx;
    }
  };
  auto load_g = [&](int i) {
    // columns past Ntot only exist in the last n tile of a padded Ntot: clamp the address, zero at the store stage
    const bool ok = (n0 + g * 4 + 32 * i) < p.Ntot;
    gv[i] = *reinterpret_cast<const f32x4*>(gbase + (ok ? goffB + 128u * i : 0u));
  };
  auto load_x = [&](int q) {
    if (qscal[q]) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int d = qst[q][e];
        const int iy = pby2 + (int)(signed char)(d & 0xff), ix = pbx2 + (int)(signed char)((d >> 8) & 0xff);
        const bool ok = (int)rowvalid2 & (int)(d >= 0) & (int)((unsigned)iy < (unsigned)p.IH) & (int)((unsigned)ix < (unsigned)p.IW);
        unsigned off = (unsigned)((pn2 * qsn[q] + (iy >> qup[q]) * qsh[q] + (ix >> qup[q]) * qsw[q] + (d >> 16) * qsc[q]) * 4);
        asm volatile("" : "+v"(off));
        off = ok ? off : 0u;
        const float v = *reinterpret_cast<const float*>(qbase[q] + off);
        xv[q][e] = ok ? v : 0.f;
      }
      xok[q] = true;
    } else {
      const int tp = qtap[q];
      const int iy = pby + (int)(short)(tp & 0xffff), ix = pbx + (tp >> 16);
      xok[q] = (int)rowvalid & (int)qvec[q] & (int)((unsigned)iy < (unsigned)p.IH) & (int)((unsigned)ix < (unsigned)p.IW);
      unsigned off = (unsigned)((pn * qsn[q] + (iy >> qup[q]) * qsh[q] + (ix >> qup[q]) * qsw[q]) * 4) + qoffB[q];
      asm volatile("" : "+v"(off));            // keep the address arithmetic unconditional (no exec-masked region, no branch)
      off = xok[q] ? off : 0u;
      xv[q] = *reinterpret_cast<const f32x4*>(qbase[q] + off);
    }
  };
  char* GsB = reinterpret_cast<char*>(Gs);
  char* XsB = reinterpret_cast<char*>(Xs);
  constexpr int GBUF = 32 * BNW * 4, XBUF = 32 * BKW * 4;
  const int stG = (r * BNW + g * 4) * 4, stX = (r * BKW + g * 4) * 4, stX2 = (r2 * BKW + g2 * 4) * 4;
  bool rowvalid_st = false;      // validity of the row whose data sits in gv/xv (snapshotted at load time)
  auto store_g = [&](int b, int i) {
    f32x4 v = gv[i];
    const bool ok = (int)rowvalid_st & (int)((n0 + g * 4 + 32 * i) < p.Ntot);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = ok ? v[e] : 0.f;
    *reinterpret_cast<f32x4*>(GsB + b * GBUF + stG + i * 128) = v;
  };
  auto store_x = [&](int b, int q) {
    f32x4 v = xv[q];
    if (qscal[q]) {
      *reinterpret_cast<f32x4*>(XsB + b * XBUF + stX2 + q * 128) = v;      // zero fill already applied per element
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float t = v[e];
        if constexpr (AFF) t = fmaxf(qfloor[q], fmaf(t, xsc[q][e], xsh[q][e]));
        v[e] = xok[q] ? t : 0.f;
      }
      *reinterpret_cast<f32x4*>(XsB + b * XBUF + stX + q * 128) = v;
    }
  };

  constexpr int NM = 16 * NI * KI;                 // MFMAs per 32-pixel step
  constexpr int PS = NI * KI;                      // MFMAs per pixel pair
  constexpr int NS = GR + 4;                       // store-stage items
  constexpr int SSTEP = (NM >= 4 * NS) ? 2 : 1;
  constexpr int S0 = NM - SSTEP * NS;

  const int nsteps = (m_end > m_begin) ? (m_end - m_begin + 31) / 32 : 0;
  if (nsteps > 0) {
    decode_pixel(m_begin);
    rowvalid_st = rowvalid;
#pragma unroll
    for (int i = 0; i < GR; ++i) load_g(i);
#pragma unroll
    for (int q = 0; q < 4; ++q) load_x(q);
#pragma unroll
    for (int i = 0; i < GR; ++i) store_g(0, i);
#pragma unroll
    for (int q = 0; q < 4; ++q) store_x(0, q);
  }
  __syncthreads();
  const int frG = ((lane >> 5) * BNW + wn * WNn + (lane & 31)) * 4;
  const int frX = ((lane >> 5) * BKW + wk * WKk + (lane & 31)) * 4;
  for (int st = 0; st < nsteps; ++st) {
    const int buf = st & 1;
    const int mnext = m_begin + (st + 1 < nsteps ? st + 1 : st) * 32;   // last step re-fetches itself into the idle buffer
    const char* Gb = GsB + buf * GBUF + frG;
    const char* Xb = XsB + buf * XBUF + frX;
    float fa[2][NI], fb[2][KI];
#pragma unroll
    for (int i = 0; i < NI; ++i) fa[0][i] = *reinterpret_cast<const float*>(Gb + i * 128);
#pragma unroll
    for (int j = 0; j < KI; ++j) fb[0][j] = *reinterpret_cast<const float*>(Xb + j * 128);
    __builtin_amdgcn_sched_barrier(0);
    static_for<NM>([&](auto mc) __attribute__((always_inline)) {
      constexpr int m = decltype(mc)::value;
      constexpr int s2 = m / PS, ij = m % PS;
      constexpr int i = ij / KI, j = ij % KI;
      constexpr int cur = s2 & 1, nxt = cur ^ 1;
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[cur][i], fb[cur][j], acc[i][j], 0, 0, 0);
      // ---- side work of this slot
      if (m == 0) { decode_pixel(mnext); }
      if (m >= 1 && m < 1 + GR) load_g(m - 1);
      if (m >= 1 + GR && m < 5 + GR) load_x(m - 1 - GR);
      if constexpr (s2 < 15) {     // fragments of the next pixel pair, spread over this pair's slots
        if constexpr (PS >= NI + KI) {
          if constexpr (ij < NI) fa[nxt][ij] = *reinterpret_cast<const float*>(Gb + (s2 + 1) * 2 * BNW * 4 + ij * 128);
          else if constexpr (ij < NI + KI) fb[nxt][ij - NI] = *reinterpret_cast<const float*>(Xb + (s2 + 1) * 2 * BKW * 4 + (ij - NI) * 128);
        } else if constexpr (ij == 0) {
#pragma unroll
          for (int a = 0; a < NI; ++a) fa[nxt][a] = *reinterpret_cast<const float*>(Gb + (s2 + 1) * 2 * BNW * 4 + a * 128);
#pragma unroll
          for (int b = 0; b < KI; ++b) fb[nxt][b] = *reinterpret_cast<const float*>(Xb + (s2 + 1) * 2 * BKW * 4 + b * 128);
        }
      }
      if (m >= S0 && (m - S0) % SSTEP == 0) {
        const int it = (m - S0) / SSTEP;
        if (it == 0) rowvalid_st = rowvalid;
        if (it < GR) store_g(buf ^ 1, it);
        else if (it < NS) store_x(buf ^ 1, it - GR);
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    __syncthreads();
  }

  float* ws = p.ws + (long long)split * p.Npad * Kp;
#pragma unroll
  for (int j = 0; j < KI; ++j) {
    const int k = kt * BKW + wk * WKk + j * 32 + (lane & 31);
    if (k >= Kp) continue;
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int n = n0 + wn * WNn + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        ws[(long long)n * Kp + k] = acc[i][j][reg];
      }
  }
}

// packed (n, k) -> framework weight index, or -1 for a padding slot
__device__ __forceinline__ long long packed_to_framework(const IgemmParams& p, const KPhase& ph, int n, int k) {
  if (n >= p.Ntot) return -1;
  int s = 0, kl = k;
  for (int i = 0; i < p.n_in - 1; ++i) {
    int span = ((ph.ntaps * p.in[i].C + kChunk - 1) / kChunk) * kChunk;
    if (s == i && kl >= span) {
      kl -= span;
      s = i + 1;
    }
  }
  const int C = p.in[s].C;
  const int j = kl / C, c = kl - j * C;
  if (j >= ph.ntaps) return -1;
  const int cc = p.in[s].ch_off + c;
  const int r = p.tr[ph.tap0 + j], t = p.ts[ph.tap0 + j];
  const long long rs = (long long)p.R * p.S;
  const long long base = p.n_is_dim0 ? ((long long)n * p.D1 + cc) : ((long long)cc * p.D1 + n);
  return base * rs + r * p.S + t;
}

__device__ __forceinline__ void pack_weights_body(const IgemmParams& p, const float* __restrict__ w, float* __restrict__ wp, long long total) {
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total; idx += (long long)gridDim.x * blockDim.x) {
    int z = 0;
    while (z + 1 < p.nphases && idx >= p.ph[z + 1].w_off) ++z;
    const KPhase& ph = p.ph[z];
    const long long local = idx - ph.w_off;
    const int Kp = ph.nchunks * kChunk;
    const int n = (int)(local / Kp), k = (int)(local - (long long)n * Kp);
    const long long src = packed_to_framework(p, ph, n, k);
    wp[idx] = src >= 0 ? w[src] : 0.f;
  }
}

__global__ void pack_weights_kernel(const IgemmParams p, const float* __restrict__ w, float* __restrict__ wp, long long total) {
  pack_weights_body(p, w, wp, total);
}

__global__ void pack_weights_many_kernel(const PackEntry* __restrict__ tab) {
  const PackEntry& e = tab[blockIdx.y];
  pack_weights_body(e.p, e.w, e.wp, e.total);
}

// 64 consecutive packed elements per block (coalesced 256-byte rows of every split slab); the four waves take the splits z = w, w + 4,
// ... and meet through LDS in a fixed order (deterministic).  The thin full-resolution layers have a few thousand weights and hundreds
// of splits: one thread per element walking all of them serially ran 10 blocks for up to 90 us.
// NW waves per block: 4 for the tiled kernels' handful of splits, 16 for the hundreds of block slabs of the persistent thin-layer
// kernels (round 4: 40 blocks of 4 waves walking 128 slabs each took 30-60 us per launch, as long as half the kernel they follow); a
// wave keeps four running sums (z = w + NW (4 i + u)) so that its loads are in flight four deep.  The order is fixed by the indices.
template <int NW>
__global__ void __launch_bounds__(64 * NW) wgrad_reduce_kernel(const IgemmParams p, float* __restrict__ dw) {
  __shared__ float part[NW][64];
  const KPhase& ph = p.ph[0];
  const int Kp = ph.nchunks * kChunk;
  const long long total = (long long)p.Ntot * Kp;
  const long long slab = (long long)p.Npad * Kp;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (long long base = blockIdx.x * 64ll; base < total; base += (long long)gridDim.x * 64) {
    const long long idx = base + lane;
    const bool live = idx < total;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (live) {
      int z = w;
      for (; z + 3 * NW < p.splits; z += 4 * NW) {
#pragma unroll
        for (int u = 0; u < 4; ++u) s[u] += p.ws[(z + u * NW) * slab + idx];
      }
#pragma unroll
      for (int u = 0; u < 3; ++u)
        if (z + u * NW < p.splits) s[u] += p.ws[(z + u * NW) * slab + idx];
    }
    part[w][lane] = (s[0] + s[1]) + (s[2] + s[3]);
    __syncthreads();
    if (w == 0 && live) {
      float tot = part[0][lane];
#pragma unroll
      for (int q = 1; q < NW; ++q) tot += part[q][lane];
      const int n = (int)(idx / Kp), k = (int)(idx - (long long)n * Kp);
      const long long dst = packed_to_framework(p, ph, n, k);
      if (dst >= 0) dw[dst] = tot;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------------ launchers
template <int BNW, int WNn, int WKk, bool ALLVEC>
static int launch_wgrad_v(const IgemmParams& p, hipStream_t stream) {
  const size_t lds = (size_t)(2 * 32 * BNW + 2 * 32 * 128) * sizeof(float) + kMaxTaps * sizeof(int);
  auto kernel = igemm_wgrad_kernel<BNW, WNn, WKk, ALLVEC>;
  int rc = enable_big_lds(kernel, lds);
  if (rc != DN_OK) return rc;
  dim3 grid((p.ph[0].nchunks + 3) / 4, p.Npad / BNW, p.splits);
  DN_LAUNCH(kernel, grid, dim3(256), lds, stream, p);
  set_last_kernel("dn::igemm_wgrad_kernel<%d, %d, %d, %s>", BNW, WNn, WKk, ALLVEC ? "true" : "false");
  return check_launch("igemm_wgrad_kernel");
}

template <int BNW, int WNn, int WKk, bool AFF>
static int launch_wgrad_u32(const IgemmParams& p, hipStream_t stream) {
  const size_t lds = (size_t)(2 * 32 * BNW + 2 * 32 * 128) * sizeof(float);
  auto kernel = igemm_wgrad_u32_kernel<BNW, WNn, WKk, AFF>;
  int rc = enable_big_lds(kernel, lds);
  if (rc != DN_OK) return rc;
  const int total = ((p.ph[0].nchunks + 3) / 4) * (p.Npad / BNW) * p.splits;
  dim3 grid((total + 7) / 8 * 8);
  DN_LAUNCH(kernel, grid, dim3(256), lds, stream, p);
  set_last_kernel("dn::igemm_wgrad_u32_kernel<%d, %d, %d, %s>", BNW, WNn, WKk, AFF ? "true" : "false");
  return check_launch("igemm_wgrad_u32_kernel");
}

template <int BNW, int WNn, int WKk>
static int launch_wgrad(const IgemmParams& p, hipStream_t stream) {
  if (p.wg_uniform)
    return p.any_affine ? launch_wgrad_u32<BNW, WNn, WKk, true>(p, stream) : launch_wgrad_u32<BNW, WNn, WKk, false>(p, stream);
  return p.allvec ? launch_wgrad_v<BNW, WNn, WKk, true>(p, stream) : launch_wgrad_v<BNW, WNn, WKk, false>(p, stream);
}

// Pixel splits of the weight gradient.  Every block does the same amount of work and the chip holds `slots` blocks at once
// (256 CUs x blocks per CU, LDS-limited), so the launch should fill a whole number of rounds from below: tiles * splits just
// under R * slots (1026 blocks on 1024 slots run as THREE rounds, measured 103 vs 135 TFLOP/s).  Fewest rounds that reach
// 92 % slot use wins (fewer splits = fewer partial slabs for wgrad_reduce_kernel).
void choose_splits(IgemmParams* p) {
  const int tiles = ((p->ph[0].nchunks + 3) / 4) * (p->Npad / p->BN);
  const int per_cu = p->BN >= 128 ? 2 : 3;      // LDS (128-wide) resp. registers (narrower tiles) limit the blocks per CU
  const int slots = 256 * per_cu;
  int max_by_work = (p->M + 255) / 256;  // at least 8 steps of 32 pixels per split
  if (max_by_work < 1) max_by_work = 1;
  int best = 1;
  double best_util = 0.0;
  for (int R = 1; R <= 4; ++R) {
    int sp = (R * slots) / tiles;
    if (sp < 1) continue;
    if (sp > max_by_work) sp = max_by_work;
    const double util = (double)tiles * sp / ((double)((tiles * sp + slots - 1) / slots) * slots);
    if (util > best_util + 1e-9) {
      best_util = util;
      best = sp;
    }
    if (util >= 0.92) break;
  }
  int per = (p->M + best - 1) / best;
  per = (per + 31) / 32 * 32;
  p->m_per_split = per;
  p->splits = (p->M + per - 1) / per;
}

// workspace of the tiled weight-gradient kernels: one [Npad][Kp] slab per split (after choose_splits)
size_t generic_wgrad_workspace_bytes(const IgemmParams& p) {
  return (size_t)p.splits * p.Npad * p.ph[0].nchunks * kChunk * sizeof(float);
}

int launch_wgrad_reduce(const IgemmParams& p, float* dw, hipStream_t stream) {
  const long long total = (long long)p.Ntot * p.ph[0].nchunks * kChunk;
  int blocks = (int)((total + 63) / 64);
  if (blocks > 8192) blocks = 8192;
  if (p.splits >= 32) DN_LAUNCH(wgrad_reduce_kernel<16>, dim3(blocks), dim3(1024), 0, stream, p, dw);
  else DN_LAUNCH(wgrad_reduce_kernel<4>, dim3(blocks), dim3(256), 0, stream, p, dw);
  return check_launch("wgrad_reduce_kernel");
}

// The tiled weight-gradient kernels + their fixed-order split sum (every layer the Winograd / thin / head kernels do not take).
int generic_wgrad(const dn_conv_desc* fwd, IgemmParams& p, const float* dy, float* dw, void* workspace, size_t workspace_bytes,
                  hipStream_t s) {
  int rc = DN_OK;
  choose_splits(&p);
  const size_t need = generic_wgrad_workspace_bytes(p);
  DN_REQUIRE(workspace_bytes >= need, DN_ERR_WORKSPACE, "wgrad workspace too small: %zu < %zu", workspace_bytes, need);
  p.ws = reinterpret_cast<float*>(workspace);
  if (fwd->kind == DN_CONV_FWD) {
    p.g = dy;  // [N*OH*OW][Cout]
    for (int i = 0; i < p.n_in; ++i) DN_REQUIRE(p.in[i].p != nullptr, DN_ERR_BAD_ARG, "operand %d has no data", i);
  } else {
    // conv-transpose: G = forward input x [N*IH*IW][Cin] (dense NHWC), gathered operand = dy [N][OH][OW][Cout]
    const dn_operand& x = fwd->in[0];
    DN_REQUIRE(x.data != nullptr && x.stride_c == 1 && x.stride_w == x.C && x.stride_h == (int64_t)fwd->IW * x.C &&
                   x.stride_n == (int64_t)fwd->IH * fwd->IW * x.C,
               DN_ERR_UNSUPPORTED, "conv-transpose wgrad needs a dense NHWC input");
    p.g = x.data;
    KOperand& o = p.in[0];
    const int co = o.C;
    o.p = dy;
    o.scale = o.shift = nullptr;
    o.sc = 1;
    o.sw = co;
    o.sh = (long long)fwd->OW * co;
    o.sn = (long long)fwd->OH * fwd->OW * co;
    o.up = 0;
    o.vec = (co % 4 == 0 && (reinterpret_cast<uintptr_t>(dy) & 15) == 0) ? 1 : 0;
    o.mC = fastdiv_magic((unsigned)co);
    o.small = ((long long)fwd->N * o.sn < (1ll << 31)) ? 1 : 0;
    p.allvec = (o.vec && o.small) ? 1 : 0;
    p.any_affine = 0;
    p.wg_uniform = (p.allvec && co % 32 == 0 && p.ph[0].ntaps <= 32 && (long long)fwd->N * o.sn * 4 + 64 < (1ll << 31)) ? 1 : 0;
  }
  // the G operand must be float4-addressable with int32 offsets too
  if (!(p.Ntot % 4 == 0 && (reinterpret_cast<uintptr_t>(p.g) & 15) == 0 && (long long)p.M * p.Ntot < (1ll << 31))) p.allvec = 0;
  // the G operand must be float4-addressable with 32-bit BYTE offsets for the fast kernel
  if (!(p.Ntot % 4 == 0 && (reinterpret_cast<uintptr_t>(p.g) & 15) == 0) || (long long)p.M * p.Ntot * 4 + 64 >= (1ll << 31)) p.wg_uniform = 0;
  if (wgrad_x3_eligible(p)) {
    rc = launch_wgrad_x3(p, s);           // fp32 products on the bf16 matrix cores (dn_wgrad_x3.hip)
  } else {
    switch (p.BN) {
      case 128: rc = launch_wgrad<128, 64, 64>(p, s); break;
      case 64: rc = launch_wgrad<64, 64, 32>(p, s); break;
      default: rc = launch_wgrad<32, 32, 32>(p, s); break;
    }
  }
  if (rc != DN_OK) return rc;
  return launch_wgrad_reduce(p, dw, s);
}

// the direct weight re-lay of one layer, and of the n leading rows of a dn_pack_many table
int launch_direct_pack(const IgemmParams& p, const float* w, float* wp, hipStream_t stream) {
  const long long total = direct_packed_elems(p);
  if (total == 0) return DN_OK;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  DN_LAUNCH(pack_weights_kernel, dim3(blocks), dim3(256), 0, stream, p, w, wp, total);
  return check_launch("pack_weights_kernel");
}

int launch_direct_pack_many(const PackEntry* tab_dev, int n, hipStream_t stream) {
  DN_LAUNCH(pack_weights_many_kernel, dim3(knobs().pack_blocks, n), dim3(256), 0, stream, tab_dev);
  return check_launch("pack_weights_many_kernel");
}

}  // namespace dn
