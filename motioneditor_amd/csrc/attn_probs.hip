// Head-mean softmax probabilities of the text cross-attention (include/motioned_probe.h), on MFMA (gfx950).
//
// The reference's editors keep attn.reshape(-1, heads, N, 77).mean(1) of every 16 x 16 cross-attention (attn_control/fully_control.py:430-432); me_attn
// never holds a normalised probability (online softmax, the division happens on the output), so the map is one more pass over Q against the <= 128 text
// keys:
//     P[row, key] = beta P[row, key] + alpha / heads * sum_h softmax_key(scale q_h . k_h)
//   * block = (item, 64 queries), wave w owns 16 of them with the query on the lane; the heads walk in ascending order (fixed: two calls are bitwise equal).
//   * per head the item's keys are staged in LDS as a [128][dh padded to 32s] tile (pad columns and rows >= nk stay zero); S^T = K Q^T puts a query's
//     128 logits into 32 registers of the four lanes that share it, so the row maximum and the row sum cost two permlane swaps each.  The loads of head
//     h + 1 (keys and the wave's own Q fragment) are in flight during the MFMAs and the softmax of head h.
//   * the head mean lives in 32 registers per lane.  After the last head it goes through the same LDS bytes once, transposed, so that a wave stores (and
//     with beta != 0 reads) 256 contiguous bytes of one output row at a time.  beta == 0 issues no load of P.
#include "me_common.h"
#include <stdio.h>
#include "../../include/motioned_probe.h"

extern "C" void me_set_error(const char* msg);
extern "C" void me_set_hip_error(const char* what, int err);
extern "C" void me_set_kernel(const char* name);

namespace {

constexpr float LOG2E = 1.4426950408889634f;
constexpr int MAXK = 128;   // keys per item at most: 8 MFMA tiles of 16
constexpr int NT = MAXK / 16;
constexpr int QB = 64;      // queries per block
constexpr int OLD = MAXK + 4;   // row stride (floats) of the transposed output image

struct probs_args {
  const f16* Q;
  const f16* K;
  float* P;
  const int* kv_item;
  long hq, hk;   // element offset from one head to the next
  int ldq, ldk, ldp;
  int heads, n_items, nq, nk, q_items;
  float scale, w, beta;   // w = alpha / heads
};

template <int DH>
__global__ __launch_bounds__(256) void attn_probs_kernel(const probs_args a) {
  constexpr int D32 = (DH + 31) / 32, CH = DH / 8;
  constexpr int RLD = D32 * 32 + 8;   // key tile [key][d], halves
  constexpr int KBYTES = MAXK * RLD * 2, OBYTES = 4 * 16 * OLD * 4;
  __shared__ __attribute__((aligned(16))) unsigned char smem[KBYTES > OBYTES ? KBYTES : OBYTES];
  f16* sK = reinterpret_cast<f16*>(smem);
  float* sO = reinterpret_cast<float*>(smem);

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;

  const int nqb = (a.nq + QB - 1) / QB;
  const int item = blockIdx.x / nqb, qb = blockIdx.x - item * nqb;
  const int qitem = a.q_items > 0 ? item % a.q_items : item;
  const int nk = a.nk;
  const int nt = (nk + 15) >> 4;
  const long krow0 = (long)a.kv_item[item] * nk;

  for (int i = tid; i < MAXK * RLD; i += 256) sK[i] = (f16)0.f;

  // this lane's query; its head slice is operand B of S^T[key, q] = K Q^T
  const int q = qb * QB + wave * 16 + l15;
  const bool qok = q < a.nq;
  const f16* qp = a.Q + ((long)qitem * a.nq + (qok ? q : 0)) * a.ldq;

  constexpr int NCHK = (MAXK * CH + 255) / 256;
  U128 rk[NCHK];
  f16x8 fqn[D32];
  auto fetch = [&](int h) {
#pragma unroll
    for (int n = 0; n < NCHK; ++n) {
      const int ci = tid + 256 * n;
      const int key = ci / CH, cc = ci - key * CH;
      rk[n].u = ci < nk * CH ? ldg128(a.K + (krow0 + key) * a.ldk + h * a.hk + cc * 8) : zero128();
    }
#pragma unroll
    for (int ks = 0; ks < D32; ++ks) {
      const int d = ks * 32 + g * 8;
      U128 u;
      u.u = (qok && d < DH) ? ldg128(qp + h * a.hq + d) : zero128();
      fqn[ks] = u.h;
    }
  };

  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  fetch(0);
  __syncthreads();   // the zero fill is done
  for (int h = 0; h < a.heads; ++h) {
#pragma unroll
    for (int n = 0; n < NCHK; ++n) {
      const int ci = tid + 256 * n;
      if (ci < nk * CH) {
        const int key = ci / CH, cc = ci - key * CH;
        *reinterpret_cast<uint4*>(sK + key * RLD + cc * 8) = rk[n].u;
      }
    }
    f16x8 fq[D32];
#pragma unroll
    for (int ks = 0; ks < D32; ++ks) fq[ks] = fqn[ks];
    __syncthreads();
    if (h + 1 < a.heads) fetch(h + 1);

    // lane (q = l15, g), reg r of tile t <-> key t * 16 + g * 4 + r
    f32x4 st[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      st[t] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (t < nt) {
#pragma unroll
        for (int ks = 0; ks < D32; ++ks) {
          const f16x8 ak = *reinterpret_cast<const f16x8*>(sK + (t * 16 + l15) * RLD + ks * 32 + g * 8);
          st[t] = mfma16(ak, fq[ks], st[t]);
        }
      }
    }
    // fp32 softmax over the nk keys, the row maximum subtracted.  Key 0 is real for every query (the pad queries too): the maximum is finite.
    // All 8 tiles, straight-line: the pad keys and the tiles past nk weigh 2^(-huge) = 0.  Skipping the 3 pad tiles of 77 keys behind uniform branches
    // measured 20 - 25 % SLOWER at dh 40 / 80.
    float mx = -1.0e30f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t][r] = (t * 16 + g * 4 + r < nk) ? st[t][r] * a.scale : -1.0e30f;
        mx = fmaxf(mx, st[t][r]);
      }
    mx = xor32_max(xor16_max(mx));
    float ls = 0.f;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[t][r] = __builtin_amdgcn_exp2f((st[t][r] - mx) * LOG2E);
        ls += st[t][r];
      }
    ls = xor32_sum(xor16_sum(ls));
    const float inv = 1.0f / ls;   // ls >= 1: the maximum's own term
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[t][r] = fmaf(st[t][r], inv, acc[t][r]);
    __syncthreads();   // every wave is done with this head's keys
  }

  // the wave's 16 x nk means, transposed through LDS: row q, then keys along the lanes
  float* sOw = sO + wave * 16 * OLD;
#pragma unroll
  for (int t = 0; t < NT; ++t)
    if (t < nt) *reinterpret_cast<float4*>(sOw + l15 * OLD + t * 16 + g * 4) = make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
  __syncthreads();
  const int q0 = qb * QB + wave * 16;
  for (int qi = 0; qi < 16 && q0 + qi < a.nq; ++qi) {
    float* prow = a.P + ((long)item * a.nq + q0 + qi) * a.ldp;
    for (int key = lane; key < nk; key += 64) {
      float v = a.w * sOw[qi * OLD + key];
      if (a.beta != 0.f) v = fmaf(a.beta, prow[key], v);
      prow[key] = v;
    }
  }
}

template <int DH>
int launch_probs(const probs_args& a, hipStream_t st) {
  const unsigned blocks = (unsigned)((long)a.n_items * ((a.nq + QB - 1) / QB));
  (void)hipGetLastError();   // drop stale errors left by other HIP users in this thread
  hipLaunchKernelGGL((attn_probs_kernel<DH>), dim3(blocks), dim3(256), 0, st, a);
  char nm[48];
  snprintf(nm, sizeof(nm), "attn_probs_kernel<%d>", DH);
  me_set_kernel(nm);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) { me_set_hip_error("me_attn_probs", (int)e); return ME_EHIP; }
  return ME_OK;
}

}  // namespace

extern "C" int me_attn_probs(const me_attn_probs_args* a, void* stream) {
  if (!a || !a->Q || !a->K || !a->P || !a->kv_item) { me_set_error("me_attn_probs: null pointer"); return ME_EINVAL; }
  if (a->dh != 40 && a->dh != 80 && a->dh != 160) { me_set_error("me_attn_probs: head dim must be 40, 80 or 160"); return ME_EINVAL; }
  if (a->nk < 1 || a->nk > MAXK) { me_set_error("me_attn_probs: nk must be 1 .. 128"); return ME_EINVAL; }
  if (a->heads <= 0 || a->n_items <= 0 || a->nq <= 0) { me_set_error("me_attn_probs: bad sizes (heads, n_items, nq > 0)"); return ME_EINVAL; }
  if (a->ldp < a->nk) { me_set_error("me_attn_probs: ldp must be >= nk"); return ME_EINVAL; }
  if (a->ldq <= 0 || a->ldk <= 0 || a->ldq % 8 || a->ldk % 8) { me_set_error("me_attn_probs: row strides ldq, ldk must be positive multiples of 8"); return ME_EINVAL; }
  if (a->hsq < 0 || a->hsk < 0 || a->hsq % 8 || a->hsk % 8) { me_set_error("me_attn_probs: head strides hsq, hsk must be multiples of 8 (0: column slices)"); return ME_EINVAL; }
  if ((((uintptr_t)a->Q | (uintptr_t)a->K) & 15) || (((uintptr_t)a->P | (uintptr_t)a->kv_item) & 3)) {
    me_set_error("me_attn_probs: misaligned pointer (Q, K 16 bytes; P, kv_item 4 bytes)");
    return ME_EINVAL;
  }
  if (a->q_items < 0) { me_set_error("me_attn_probs: q_items must be >= 0"); return ME_EINVAL; }
  if ((long)a->n_items * a->nq * a->heads > 0x7fffffffL) { me_set_error("me_attn_probs: n_items * nq * heads must stay below 2^31"); return ME_EINVAL; }
  probs_args k;
  k.Q = reinterpret_cast<const f16*>(a->Q);
  k.K = reinterpret_cast<const f16*>(a->K);
  k.P = a->P;
  k.kv_item = a->kv_item;
  k.hq = a->hsq ? a->hsq : a->dh;
  k.hk = a->hsk ? a->hsk : a->dh;
  k.ldq = a->ldq; k.ldk = a->ldk; k.ldp = a->ldp;
  k.heads = a->heads; k.n_items = a->n_items; k.nq = a->nq; k.nk = a->nk; k.q_items = a->q_items;
  k.scale = a->scale;
  k.w = a->alpha * (1.0f / (float)a->heads);
  k.beta = a->beta;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  switch (a->dh) {
    case 40: return launch_probs<40>(k, st);
    case 80: return launch_probs<80>(k, st);
    default: return launch_probs<160>(k, st);
  }
}
