// Backward of the causal temporal attention for clips of 65 .. 256 frames (plain row order, row = (b * frames + frame) * npix + pixel), on MFMA (gfx950).
//
// The reference differentiates TemporalSelfAttention._attention with torch autograd (null-text optimisation, adapter training, stage-1 tuning).  The
// forward (csrc/tattn.hip tattn_long_kernel) stashes no log-sum-exp, so the backward rebuilds its softmax statistics:
//     P = 2^(s c - lse),  dP = dO V^T,  delta_i = sum_j P_ij dP_ij,  dS = P o (dP - delta),  dV = P^T dO,  dK = scale dS^T Q,  dQ = scale dS K
// in two deterministic kernels after csrc/attn_bwd.hip (no atomics; every output element has one owner and is WRITTEN, =):
//   * tattn_bwd_long_dq_kernel, query-centric: a block owns 64 query frames of one (batch entry, pixel, head), a wave 16 of them, the query on the lane.
//     Sweep 1 walks the key stages 0 .. diagonal: S^T = K Q^T, dP^T = V dO^T, an online softmax per query (running maximum m, running sum l) with
//     dl = sum_j 2^(s_j - m) dP_j accumulated beside l under the same rescale; lse = m + log2 l and delta = dl / l go to the caller's scratch.
//     Sweep 2 walks the same stages again: dS^T packed to fp16 as operand B of dQ^T[d, q] += K^T[d, key] dS^T[key, q].
//   * tattn_bwd_long_dkv_kernel, key-centric: a block owns 64 key frames (a wave 16, K / V fragments in registers as operand B) and walks the query
//     stages from its own diagonal to the last frame, 32 queries per stage, with lse / delta from the scratch: dV^T += dO^T P, dK^T += Q^T dS.
// A block takes ONE head (a 40 / 80 / 160-column slice), not the forward's 320 columns: own K / V plus streamed Q / dO of 320 columns do not fit the LDS.
// dO reaches the MFMAs rounded to fp16 and delta is a sum over products of that same rounded dO: a query whose dO row is zero gets dP = 0, delta = 0 and
// an exactly zero dQ row.  Rows >= frames of the last stage are neither read nor written: they are zero tiles in LDS, removed by the causal mask.
#include "me_common.h"
#include <stdio.h>
#include "../../include/motioned_long.h"

extern "C" void me_set_error(const char* msg);
extern "C" void me_set_hip_error(const char* what, int err);
extern "C" void me_set_kernel(const char* name);

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int MIN_FRAMES = 65, MAX_FRAMES = 256;
constexpr int BLK = 64;   // query frames per block of the dq kernel, key frames per block of the dkv kernel

struct tbl_args {
  const f16* Q;
  const f16* K;
  const f16* V;
  const float* dO;
  float* dQ;
  float* dK;
  float* dV;
  float* lse;     // [rows][heads], log2 domain
  float* delta;   // [rows][heads]
  int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
  int batch, frames, npix, heads;
  float scale;
};

__device__ __forceinline__ uint4 f32x8_to_f16(const float* p) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  U128 u;
  u.e[0] = (f16)a.x; u.e[1] = (f16)a.y; u.e[2] = (f16)a.z; u.e[3] = (f16)a.w;
  u.e[4] = (f16)b.x; u.e[5] = (f16)b.y; u.e[6] = (f16)b.z; u.e[7] = (f16)b.w;
  return u.u;
}

// ---- lse, delta, dQ: block = (batch entry, pixel, head, 64 query frames); wave w owns 16 queries; keys walk through LDS KT at a time ----
template <int DH, int KT>   // KT keys per stage (64; 32 at dh 160 so that the three tiles stay inside 64 KB of LDS)
__global__ __launch_bounds__(256) void tattn_bwd_long_dq_kernel(const tbl_args a) {
  constexpr int D32 = (DH + 31) / 32, DT = (DH + 15) / 16, CH = DH / 8;
  constexpr int NT = KT / 16, NKK = KT / 32;
  constexpr int RLD = D32 * 32 + 8;       // row-major K / V tiles [key][d]
  constexpr int TLD = KT + 8;             // transposed K tile [d][key slot]
  __shared__ __attribute__((aligned(16))) f16 sK[KT * RLD];
  __shared__ __attribute__((aligned(16))) f16 sV[KT * RLD];
  __shared__ __attribute__((aligned(16))) f16 sKt[DT * 16 * TLD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;

  const int F = a.frames;
  const int nqb = (F + BLK - 1) / BLK;
  int w = blockIdx.x;
  const int qb = w % nqb;                 // the query blocks of one (batch entry, pixel, head) are neighbours, then the heads of a pixel
  w /= nqb;
  const int h = w % a.heads;
  w /= a.heads;
  const int p = w % a.npix;
  const int b = w / a.npix;
  const long frow0 = (long)b * F * a.npix + p;   // frame j of this (batch entry, pixel) is row frow0 + j * npix

  for (int i = tid; i < KT * RLD; i += 256) { sK[i] = (f16)0.f; sV[i] = (f16)0.f; }
  for (int i = tid; i < DT * 16 * TLD; i += 256) sKt[i] = (f16)0.f;

  // this lane's query: Q and dO fragments as MFMA operand B
  const int q = qb * BLK + wave * 16 + l15;
  const bool qok = q < F;
  const long qrow = frow0 + (long)(qok ? q : 0) * a.npix;
  f16x8 fq[D32], fdo[D32];
#pragma unroll
  for (int ks = 0; ks < D32; ++ks) {
    const int d = ks * 32 + g * 8;
    U128 uq, ud;
    uq.u = (qok && d < DH) ? ldg128(a.Q + qrow * a.ldq + h * DH + d) : zero128();
    ud.u = (qok && d < DH) ? f32x8_to_f16(a.dO + qrow * a.lddo + h * DH + d) : zero128();
    fq[ks] = uq.h;
    fdo[ks] = ud.h;
  }
  const float c = a.scale * LOG2E;
  __syncthreads();

  // Stages = KT-key tiles from frame 0 to the tile that holds the diagonal of the block's last real query; the loads of stage s + 1 are in flight
  // during the MFMAs of stage s (csrc/attn_bwd.hip).
  constexpr int NCHK = (KT * CH + 255) / 256;
  const int last = qb * BLK + BLK - 1 < F ? qb * BLK + BLK - 1 : F - 1;
  const int nstage = last / KT + 1;
  U128 rk[NCHK], rv[NCHK];
  auto fetch = [&](int sidx) {
    const int kt0 = sidx * KT;
#pragma unroll
    for (int n = 0; n < NCHK; ++n) {
      const int ci = tid + 256 * n;
      const int key = ci / CH, cc = ci - key * CH;
      const bool ok = ci < KT * CH && kt0 + key < F;
      const long row = frow0 + (long)(kt0 + key) * a.npix;
      rk[n].u = ok ? ldg128(a.K + row * a.ldk + h * DH + cc * 8) : zero128();
      rv[n].u = ok ? ldg128(a.V + row * a.ldv + h * DH + cc * 8) : zero128();
    }
  };
  // K row-major and transposed (key slot order), V row-major
  auto stage = [&]() {
#pragma unroll
    for (int n = 0; n < NCHK; ++n) {
      const int ci = tid + 256 * n;
      if (ci < KT * CH) {
        const int key = ci / CH, cc = ci - key * CH;
        *reinterpret_cast<uint4*>(sK + key * RLD + cc * 8) = rk[n].u;
        *reinterpret_cast<uint4*>(sV + key * RLD + cc * 8) = rv[n].u;
        // key kk * 32 + i * 16 + g * 4 + r sits at slot kk * 32 + g * 8 + i * 4 + r
        const int pos = (key & 32) | ((key & 12) << 1) | ((key & 16) >> 2) | (key & 3);
#pragma unroll
        for (int e = 0; e < 8; ++e) sKt[(cc * 8 + e) * TLD + pos] = rk[n].e[e];
      }
    }
  };
  // S^T[key, q] = K Q^T, dP^T[key, q] = V dO^T: lane (q = l15, g), reg r <-> key t * 16 + g * 4 + r
  f32x4 st[NT], dpt[NT];
  auto scores = [&]() {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      dpt[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < D32; ++ks) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        const f16x8 ak = *reinterpret_cast<const f16x8*>(sK + (t * 16 + l15) * RLD + ks * 32 + g * 8);
        const f16x8 av = *reinterpret_cast<const f16x8*>(sV + (t * 16 + l15) * RLD + ks * 32 + g * 8);
        st[t] = mfma16(ak, fq[ks], st[t]);
        dpt[t] = mfma16(av, fdo[ks], dpt[t]);
      }
    }
  };

  // ---- sweep 1: online softmax statistics.  Every query, the pad queries too, sees key frame 0 in stage 0: m is finite from the first stage on ----
  float m = -1.0e30f, l = 0.f, dl = 0.f;   // running maximum (the lanes of a query agree); running sum and sum of P dP (this lane's keys)
  fetch(0);
  for (int sidx = 0; sidx < nstage; ++sidx) {
    const int kt0 = sidx * KT;
    stage();
    __syncthreads();
    if (sidx + 1 < nstage) fetch(sidx + 1);
    scores();
    float mx = -1.0e30f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t][r] = (kt0 + t * 16 + g * 4 + r <= q) ? st[t][r] * c : -1.0e30f;   // causal; the pad keys of the last stage lie above every real query
        mx = fmaxf(mx, st[t][r]);
      }
    mx = fmaxf(m, xor32_max(xor16_max(mx)));
    const float alpha = __builtin_amdgcn_exp2f(m - mx);   // stage 0: exp2(-1e30 - finite) = 0 on zero sums
    m = mx;
    float ls = 0.f, ds = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = __builtin_amdgcn_exp2f(st[t][r] - mx);
        ls += pv;
        ds = fmaf(pv, dpt[t][r], ds);
      }
    l = l * alpha + ls;
    dl = dl * alpha + ds;
    __syncthreads();   // every wave is done with this stage's tiles
  }
  l = xor32_sum(xor16_sum(l));
  dl = xor32_sum(xor16_sum(dl));
  const float lse_q = m + log2f(l);
  const float del_q = dl / l;
  if (qok && g == 0) {
    a.lse[qrow * a.heads + h] = lse_q;
    a.delta[qrow * a.heads + h] = del_q;
  }

  // ---- sweep 2: dQ^T[d = dt * 16 + g * 4 + r][q = l15] over the same stages ----
  f32x4 dqt[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dqt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  fetch(0);
  for (int sidx = 0; sidx < nstage; ++sidx) {
    const int kt0 = sidx * KT;
    stage();
    __syncthreads();
    if (sidx + 1 < nstage) fetch(sidx + 1);
    scores();
    // dS^T -> operand B of dQ^T[d, q] += K^T[d, key] dS^T[key, q] (k-slot (g, i * 4 + r) = key kk * 32 + i * 16 + g * 4 + r)
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) {
      U128 ud;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int t = 2 * kk + i;
          const bool ok = kt0 + t * 16 + g * 4 + r <= q;
          const float pv = ok ? __builtin_amdgcn_exp2f(st[t][r] * c - lse_q) : 0.f;
          ud.e[i * 4 + r] = (f16)(pv * (dpt[t][r] - del_q));
        }
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const f16x8 akt = *reinterpret_cast<const f16x8*>(sKt + (dt * 16 + l15) * TLD + kk * 32 + g * 8);
        dqt[dt] = mfma16(akt, ud.h, dqt[dt]);
      }
    }
    __syncthreads();
  }

  if (!qok) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + g * 4;
    if (d >= DH) continue;
    *reinterpret_cast<float4*>(a.dQ + qrow * a.lddq + h * DH + d) =
        make_float4(dqt[dt][0] * a.scale, dqt[dt][1] * a.scale, dqt[dt][2] * a.scale, dqt[dt][3] * a.scale);
  }
}

// ---- dK, dV: block = (batch entry, pixel, head, 64 key frames); wave w owns 16 keys; queries walk through LDS 32 at a time from the block's diagonal ----
template <int DH>
__global__ __launch_bounds__(256) void tattn_bwd_long_dkv_kernel(const tbl_args a) {
  constexpr int D32 = (DH + 31) / 32, DT = (DH + 15) / 16, CH = DH / 8;
  constexpr int QB = 32;                  // queries per stage
  constexpr int RLD = D32 * 32 + 8;       // row-major tiles [query][d], halves
  constexpr int TLD = QB + 8;             // transposed tiles [d][query slot], halves
  __shared__ __attribute__((aligned(16))) f16 sQ[QB * RLD];
  __shared__ __attribute__((aligned(16))) f16 sdO[QB * RLD];
  __shared__ __attribute__((aligned(16))) f16 sQt[DT * 16 * TLD];
  __shared__ __attribute__((aligned(16))) f16 sdOt[DT * 16 * TLD];
  __shared__ __attribute__((aligned(16))) float slse[QB];
  __shared__ __attribute__((aligned(16))) float sdel[QB];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;

  const int F = a.frames;
  const int nkb = (F + BLK - 1) / BLK;
  int w = blockIdx.x;
  const int kb = w % nkb;
  w /= nkb;
  const int h = w % a.heads;
  w /= a.heads;
  const int p = w % a.npix;
  const int b = w / a.npix;
  const long frow0 = (long)b * F * a.npix + p;

  for (int i = tid; i < QB * RLD; i += 256) { sQ[i] = (f16)0.f; sdO[i] = (f16)0.f; }
  for (int i = tid; i < DT * 16 * TLD; i += 256) { sQt[i] = (f16)0.f; sdOt[i] = (f16)0.f; }

  // this lane's key: K and V fragments as MFMA operand B (lane (key = l15, g) holds row[key][ks * 32 + g * 8 .. + 8])
  const int key = kb * BLK + wave * 16 + l15;
  const bool kvalid = key < F;
  const long krow = frow0 + (long)(kvalid ? key : 0) * a.npix;
  f16x8 fk[D32], fv[D32];
#pragma unroll
  for (int ks = 0; ks < D32; ++ks) {
    const int d = ks * 32 + g * 8;
    U128 uk, uv;
    uk.u = (kvalid && d < DH) ? ldg128(a.K + krow * a.ldk + h * DH + d) : zero128();
    uv.u = (kvalid && d < DH) ? ldg128(a.V + krow * a.ldv + h * DH + d) : zero128();
    fk[ks] = uk.h;
    fv[ks] = uv.h;
  }

  f32x4 dkt[DT], dvt[DT];   // dK^T, dV^T [d = dt * 16 + g * 4 + r][key = l15]
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    dkt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    dvt[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float c = a.scale * LOG2E;
  __syncthreads();

  // Stages = 32-query tiles from the block's first key frame (query stages wholly below it are never read) to the last frame.
  constexpr int NCHK = (QB * CH + 255) / 256;
  const int qs0 = kb * BLK;
  const int nstage = (F - qs0 + QB - 1) / QB;
  U128 rq[NCHK], rd[NCHK];
  float rl = 0.f, rdl = 0.f;
  auto fetch = [&](int sidx) {
    const int q0 = qs0 + sidx * QB;
#pragma unroll
    for (int n = 0; n < NCHK; ++n) {
      const int ci = tid + 256 * n;
      const int q = ci / CH, cc = ci - q * CH;
      const bool ok = ci < QB * CH && q0 + q < F;
      const long row = frow0 + (long)(q0 + q) * a.npix;
      rq[n].u = ok ? ldg128(a.Q + row * a.ldq + h * DH + cc * 8) : zero128();
      rd[n].u = ok ? f32x8_to_f16(a.dO + row * a.lddo + h * DH + cc * 8) : zero128();
    }
    if (tid < QB) {
      const bool ok = q0 + tid < F;
      const long row = frow0 + (long)(q0 + tid) * a.npix;
      rl = ok ? a.lse[row * a.heads + h] : 1.0e30f;   // frames past the last: P = 2^(-huge) = 0
      rdl = ok ? a.delta[row * a.heads + h] : 0.f;
    }
  };
  fetch(0);
  for (int sidx = 0; sidx < nstage; ++sidx) {
    const int q0 = qs0 + sidx * QB;
    // ---- stage 32 queries: Q and dO row-major and transposed (query slot order), lse, delta ----
#pragma unroll
    for (int n = 0; n < NCHK; ++n) {
      const int ci = tid + 256 * n;
      if (ci < QB * CH) {
        const int q = ci / CH, cc = ci - q * CH;
        *reinterpret_cast<uint4*>(sQ + q * RLD + cc * 8) = rq[n].u;
        *reinterpret_cast<uint4*>(sdO + q * RLD + cc * 8) = rd[n].u;
        const int pos = ((q >> 2) & 3) * 8 + (q >> 4) * 4 + (q & 3);   // query i * 16 + g * 4 + r sits at slot g * 8 + i * 4 + r
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          sQt[(cc * 8 + e) * TLD + pos] = rq[n].e[e];
          sdOt[(cc * 8 + e) * TLD + pos] = rd[n].e[e];
        }
      }
    }
    if (tid < QB) {
      slse[tid] = rl;
      sdel[tid] = rdl;
    }
    __syncthreads();
    if (sidx + 1 < nstage) fetch(sidx + 1);

    // ---- S[q, key] = Q K^T, dP[q, key] = dO V^T: lane (key = l15, g), reg r <-> query i * 16 + g * 4 + r ----
    f32x4 s[2], dp[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      s[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      dp[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int ks = 0; ks < D32; ++ks) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f16x8 aq = *reinterpret_cast<const f16x8*>(sQ + (i * 16 + l15) * RLD + ks * 32 + g * 8);
        const f16x8 ad = *reinterpret_cast<const f16x8*>(sdO + (i * 16 + l15) * RLD + ks * 32 + g * 8);
        s[i] = mfma16(aq, fk[ks], s[i]);
        dp[i] = mfma16(ad, fv[ks], dp[i]);
      }
    }
    // ---- P, dS -> fp16 operand B fragments (k-slot (g, i * 4 + r) = query i * 16 + g * 4 + r); causal: key <= query ----
    U128 up, ud;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const float4 l4 = *reinterpret_cast<const float4*>(slse + i * 16 + g * 4), d4 = *reinterpret_cast<const float4*>(sdel + i * 16 + g * 4);
      const float L[4] = {l4.x, l4.y, l4.z, l4.w}, Dl[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = kvalid && key <= q0 + i * 16 + g * 4 + r;
        const float pv = ok ? __builtin_amdgcn_exp2f(s[i][r] * c - L[r]) : 0.f;
        up.e[i * 4 + r] = (f16)pv;
        ud.e[i * 4 + r] = (f16)(pv * (dp[i][r] - Dl[r]));
      }
    }
    // ---- dV^T[d, key] += dO^T[d, q] P[q, key],  dK^T[d, key] += Q^T[d, q] dS[q, key] ----
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      const f16x8 at = *reinterpret_cast<const f16x8*>(sdOt + (dt * 16 + l15) * TLD + g * 8);
      const f16x8 aqt = *reinterpret_cast<const f16x8*>(sQt + (dt * 16 + l15) * TLD + g * 8);
      dvt[dt] = mfma16(at, up.h, dvt[dt]);
      dkt[dt] = mfma16(aqt, ud.h, dkt[dt]);
    }
    __syncthreads();   // every wave is done with this stage's tiles
  }

  if (!kvalid) return;
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) {
    const int d = dt * 16 + g * 4;
    if (d >= DH) continue;
    *reinterpret_cast<float4*>(a.dK + krow * a.lddk + h * DH + d) =
        make_float4(dkt[dt][0] * a.scale, dkt[dt][1] * a.scale, dkt[dt][2] * a.scale, dkt[dt][3] * a.scale);
    *reinterpret_cast<float4*>(a.dV + krow * a.lddv + h * DH + d) = make_float4(dvt[dt][0], dvt[dt][1], dvt[dt][2], dvt[dt][3]);
  }
}

template <int DH>
int launch_long(const tbl_args& a, hipStream_t st) {
  const unsigned blocks = (unsigned)((long)a.batch * a.npix * a.heads * ((a.frames + BLK - 1) / BLK));
  (void)hipGetLastError();   // drop stale errors left by other HIP users in this thread
  hipLaunchKernelGGL((tattn_bwd_long_dq_kernel<DH, (DH > 80 ? 32 : 64)>), dim3(blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL((tattn_bwd_long_dkv_kernel<DH>), dim3(blocks), dim3(256), 0, st, a);
  char nm[80];
  snprintf(nm, sizeof(nm), "tattn_bwd_long_dq_kernel<%d>+tattn_bwd_long_dkv_kernel<%d>", DH, DH);
  me_set_kernel(nm);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { me_set_hip_error("me_tattn_bwd_long", (int)e); return ME_EHIP; }
  return ME_OK;
}

}  // namespace

extern "C" int64_t me_tattn_bwd_long_work_bytes(int32_t batch, int32_t frames, int32_t npix, int32_t heads) {
  if (batch <= 0 || frames <= 0 || npix <= 0 || heads <= 0) return 0;
  return (int64_t)2 * sizeof(float) * batch * frames * npix * heads;   // lse and delta, one fp32 each per (row, head)
}

extern "C" int me_tattn_bwd_long(void* dq, int32_t lddq, void* dk, int32_t lddk, void* dv, int32_t lddv, const void* q, int32_t ldq, const void* k, int32_t ldk,
                                 const void* v, int32_t ldv, const void* dout, int32_t lddo, int32_t batch, int32_t frames, int32_t npix, int32_t heads, int32_t dh,
                                 float scale, void* work, int64_t work_bytes, void* stream) {
  if (!dq || !dk || !dv || !q || !k || !v || !dout) { me_set_error("me_tattn_bwd_long: null pointer"); return ME_EINVAL; }
  if (batch <= 0 || npix <= 0 || heads <= 0) { me_set_error("me_tattn_bwd_long: bad sizes (batch, npix, heads > 0)"); return ME_EINVAL; }
  if (frames < MIN_FRAMES) { me_set_error("me_tattn_bwd_long: frames must be > 64 (me_tattn_bwd serves frames <= 64)"); return ME_EINVAL; }
  if (frames > MAX_FRAMES) { me_set_error("me_tattn_bwd_long: frames must be <= 256 (the limit of the key-tiled kernels)"); return ME_EINVAL; }
  if (dh != 40 && dh != 80 && dh != 160) { me_set_error("me_tattn_bwd_long: head dim must be 40, 80 or 160"); return ME_EINVAL; }
  if (ldq % 8 || ldk % 8 || ldv % 8 || lddo % 4 || lddq % 4 || lddk % 4 || lddv % 4) {
    me_set_error("me_tattn_bwd_long: row strides must be multiples of 8 (fp16 tensors) / 4 (fp32 gradients)");
    return ME_EINVAL;
  }
  const long C = (long)heads * dh;   // rows narrower than heads * dh would overlap: two blocks would then write one gradient element
  if (ldq < C || ldk < C || ldv < C || lddo < C || lddq < C || lddk < C || lddv < C) {
    me_set_error("me_tattn_bwd_long: row strides must cover heads * dh columns");
    return ME_EINVAL;
  }
  if (((uintptr_t)q | (uintptr_t)k | (uintptr_t)v | (uintptr_t)dout | (uintptr_t)dq | (uintptr_t)dk | (uintptr_t)dv) & 15) {
    me_set_error("me_tattn_bwd_long: misaligned pointer (16 bytes)");
    return ME_EINVAL;
  }
  if (!work || ((uintptr_t)work & 15)) { me_set_error("me_tattn_bwd_long: work is null or not 16-byte aligned"); return ME_EINVAL; }
  if (work_bytes < me_tattn_bwd_long_work_bytes(batch, frames, npix, heads)) {
    me_set_error("me_tattn_bwd_long: work is smaller than me_tattn_bwd_long_work_bytes(batch, frames, npix, heads)");
    return ME_EINVAL;
  }
  const long rows = (long)batch * frames * npix;
  if (rows * heads > 0x7fffffffL) { me_set_error("me_tattn_bwd_long: batch * frames * npix * heads must stay below 2^31"); return ME_EINVAL; }
  tbl_args a;
  a.Q = reinterpret_cast<const f16*>(q);
  a.K = reinterpret_cast<const f16*>(k);
  a.V = reinterpret_cast<const f16*>(v);
  a.dO = reinterpret_cast<const float*>(dout);
  a.dQ = reinterpret_cast<float*>(dq);
  a.dK = reinterpret_cast<float*>(dk);
  a.dV = reinterpret_cast<float*>(dv);
  a.lse = reinterpret_cast<float*>(work);
  a.delta = a.lse + rows * heads;
  a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.lddo = lddo; a.lddq = lddq; a.lddk = lddk; a.lddv = lddv;
  a.batch = batch; a.frames = frames; a.npix = npix; a.heads = heads;
  a.scale = scale;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (dh) {
    case 40: return launch_long<40>(a, st);
    case 80: return launch_long<80>(a, st);
    default: return launch_long<160>(a, st);
  }
}
