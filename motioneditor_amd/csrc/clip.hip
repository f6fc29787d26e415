// CLIP text encoder kernels of libmotioned (gfx950): the three operators of transformers' CLIPTextModel that the UNet / VAE side
// of the library does not have -- token + position embedding lookup, causal short-sequence attention at head size 64, quick-GELU.
// LayerNorm and the dense projections of the encoder are me_layernorm / me_gemm.
#include "me_common.h"
#include "../../include/motioned.h"

namespace {

// out[r, :] = fp16(tok[ids[r], :] + pos[r % seq, :]); one thread = 8 columns (16-byte loads / stores), fp32 sum rounded once.
// The wrapper checks the ids on the host; an id outside [0, vocab) reaching the device reads nothing and leaves a zero row.
__global__ __launch_bounds__(256) void embed_rows_kernel(f16* __restrict__ out, const f16* __restrict__ tok, const f16* __restrict__ pos,
                                                         const int* __restrict__ ids, long rows, int seq, int C, int vocab) {
  const int vec_per_row = C >> 3;
  const long total = rows * vec_per_row;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / vec_per_row;
    const int c = (int)(idx - r * vec_per_row) << 3;
    const int id = ids[r];
    U128 o;
    o.u = zero128();
    if (id >= 0 && id < vocab) {
      U128 t, p;
      t.u = ldg128(tok + (long)id * C + c);
      p.u = ldg128(pos + (long)(r % seq) * C + c);
#pragma unroll
      for (int e = 0; e < 8; ++e) o.e[e] = (f16)((float)t.e[e] + (float)p.e[e]);
    }
    *reinterpret_cast<uint4*>(out + r * C + c) = o.u;
  }
}

// y = x * sigmoid(1.702 x) (transformers' "quick_gelu"), fp32 inside, one rounding.  Large |x|: 2^(+big) = inf -> rcp -> 0 -> x * 0;
// 2^(-big) = 0 -> x.
__device__ __forceinline__ float quick_gelu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.702f * 1.4426950408889634f * x)); }

__global__ __launch_bounds__(256) void quick_gelu_kernel(f16* Y, const f16* X, long n) {
  for (long idx = ((long)blockIdx.x * 256 + threadIdx.x) * 8; idx < n; idx += (long)gridDim.x * 256 * 8) {
    if (idx + 8 <= n) {
      U128 u, o;
      u.u = ldg128(X + idx);
#pragma unroll
      for (int e = 0; e < 8; ++e) o.e[e] = (f16)quick_gelu_f((float)u.e[e]);
      *reinterpret_cast<uint4*>(Y + idx) = o.u;
    } else {
      for (long k = idx; k < n; ++k) Y[k] = (f16)quick_gelu_f((float)X[k]);
    }
  }
}

// Causal self-attention, dh = 64, nq = nk <= 128.  Block = (sequence, head, 64-query block), 4 waves, one 16-query tile per wave.
// The block stages the keys its queries can see (0 .. last query of the block) in LDS: K row-major, V transposed.  Every wave computes
// S^T = K Q^T per 16-key tile, so that the accumulator layout (lane l, register r: key (l >> 4) * 4 + r, query l & 15) is already the
// B-operand layout of O^T = V^T P^T once two key tiles are paired into one 32-deep contraction -- slot (l >> 4) * 8 + j of the
// contraction stands for key tileA * 16 + (l >> 4) * 4 + j (j < 4) or tileB * 16 + (l >> 4) * 4 + j - 4, and the A operand reads V^T
// at the same keys -- so P never goes through LDS.  Softmax in fp32 over all visible keys at once (at most 8 tiles x 4 registers), row
// maximum subtracted; masked keys (key > query, or a key of the tile padding) get weight exactly 0 and are left out of the denominator.
constexpr int CA_DH = 64, CA_MAXN = 128, CA_QB = 64, CA_KP = CA_DH + 8, CA_VP = CA_MAXN + 8, CA_TILES = CA_MAXN / 16;

__global__ __launch_bounds__(256) void attn_causal_kernel(f16* __restrict__ O, int ldo, const f16* __restrict__ Q, int ldq, const f16* __restrict__ K, int ldk,
                                                          const f16* __restrict__ V, int ldv, int heads, int nq, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) f16 Ks[CA_MAXN * CA_KP];   // [key][d], pitch 72
  __shared__ __attribute__((aligned(16))) f16 Vt[CA_DH * CA_VP];     // [d][key], pitch 136
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const long row0 = (long)seq * nq;
  const int col0 = head * CA_DH;
  const int qb0 = blockIdx.y * CA_QB;
  const int nkeys = min(nq, qb0 + CA_QB);           // keys this block's queries can see
  const int nkeys_pad = (nkeys + 31) & ~31;         // what the paired key tiles may touch: zero-filled beyond nkeys
  const int tid = threadIdx.x;

  for (int i = tid; i < nkeys_pad * (CA_DH / 8); i += 256) {
    const int key = i >> 3, c = (i & 7) << 3;
    U128 k, v;
    k.u = zero128();
    v.u = zero128();
    if (key < nkeys) {
      k.u = ldg128(K + (row0 + key) * ldk + col0 + c);
      v.u = ldg128(V + (row0 + key) * ldv + col0 + c);
    }
    *reinterpret_cast<uint4*>(&Ks[key * CA_KP + c]) = k.u;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(c + e) * CA_VP + key] = v.e[e];
  }
  __syncthreads();

  const int wave = tid >> 6, l = tid & 63;
  const int q0 = qb0 + wave * 16;
  if (q0 >= nq) return;                              // (after the only barrier)
  const int li = l & 15, lg = l >> 4;
  const int q = q0 + li;
  const int nt = min(q0 / 16 + 1, (nkeys + 15) >> 4);   // 16-key tiles up to and including the diagonal one

  // Q^T as the B operand: lane holds Q[q][kk * 32 + lg * 8 + 0..7]; a padded query row reads as zeros
  U128 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    qf[kk].u = zero128();
    if (q < nq) qf[kk].u = ldg128(Q + (row0 + q) * ldq + col0 + kk * 32 + lg * 8);
  }

  float s[CA_TILES][4];
  float m = -3.0e38f;
#pragma unroll
  for (int t = 0; t < CA_TILES; ++t) {
    if (t < nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        U128 a;
        a.u = *reinterpret_cast<const uint4*>(&Ks[(t * 16 + li) * CA_KP + kk * 32 + lg * 8]);
        acc = mfma16(a.h, qf[kk].h, acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = t * 16 + lg * 4 + r;
        const bool ok = key <= q && key < nq;
        s[t][r] = ok ? acc[r] : -3.0e38f;
        m = fmaxf(m, s[t][r]);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[t][r] = -3.0e38f;
    }
  }
  // the 4 lanes l & 15 == li (lg = 0..3) share a query
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float sum = 0.f;
  f16 p[CA_TILES][4];
#pragma unroll
  for (int t = 0; t < CA_TILES; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int key = t * 16 + lg * 4 + r;
      const bool ok = t < nt && key <= q && key < nq;
      const float e = ok ? __builtin_amdgcn_exp2f((s[t][r] - m) * scale_log2e) : 0.f;
      sum += e;
      p[t][r] = (f16)e;
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;    // every stored query sees at least its own key: sum >= 1

  // O^T[d][q] = sum_key V^T[d][key] P^T[key][q], key tiles in pairs
  f32x4 o[CA_DH / 16];
#pragma unroll
  for (int dt = 0; dt < CA_DH / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < CA_TILES / 2; ++j) {
    if (2 * j < nt) {
      f16x8 b;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        b[r] = p[2 * j][r];
        b[4 + r] = p[2 * j + 1][r];
      }
#pragma unroll
      for (int dt = 0; dt < CA_DH / 16; ++dt) {
        const f16* vrow = &Vt[(dt * 16 + li) * CA_VP + lg * 4];
        U64 lo, hi;
        lo.u = *reinterpret_cast<const uint2*>(vrow + (2 * j) * 16);
        hi.u = *reinterpret_cast<const uint2*>(vrow + (2 * j + 1) * 16);
        f16x8 a;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          a[r] = lo.e[r];
          a[4 + r] = hi.e[r];
        }
        o[dt] = mfma16(a, b, o[dt]);
      }
    }
  }
  if (q < nq) {
#pragma unroll
    for (int dt = 0; dt < CA_DH / 16; ++dt) {   // lane l, register r: O[q][dt * 16 + lg * 4 + r]
      U64 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) w.e[r] = (f16)(o[dt][r] * inv);
      *reinterpret_cast<uint2*>(O + (row0 + q) * ldo + col0 + dt * 16 + lg * 4) = w.u;
    }
  }
}

inline unsigned grid_for(long n, long cap = 16384) {
  long b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

}  // namespace

extern "C" void me_set_error(const char* msg);
extern "C" void me_set_hip_error(const char* what, int err);
extern "C" void me_set_kernel(const char* name);

#define ME_CHECK_LAUNCH(name)                                         \
  {                                                                   \
    const hipError_t e_ = hipGetLastError();                          \
    if (e_ != hipSuccess) {                                           \
      me_set_hip_error(name ": kernel launch failed", (int)e_);       \
      return ME_EHIP;                                                 \
    }                                                                 \
  }                                                                   \
  return ME_OK;

extern "C" int me_embed_rows(void* out, const void* tok, const void* pos, const int32_t* ids, int64_t rows, int32_t seq, int32_t C, int32_t vocab, void* stream) {
  if (!out || !tok || !pos || !ids || rows <= 0 || seq <= 0 || vocab <= 0 || C <= 0 || C % 8 ||
      (((uintptr_t)out | (uintptr_t)tok | (uintptr_t)pos) & 15) || ((uintptr_t)ids & 3)) {
    me_set_error("me_embed_rows: bad arguments (C a multiple of 8, 16-byte aligned tables)");
    return ME_EINVAL;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users in this thread
  me_set_kernel("embed_rows_kernel");
  hipLaunchKernelGGL(embed_rows_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<f16*>(out),
                     reinterpret_cast<const f16*>(tok), reinterpret_cast<const f16*>(pos), reinterpret_cast<const int*>(ids), (long)rows, seq, C, vocab);
  ME_CHECK_LAUNCH("me_embed_rows")
}

extern "C" int me_quick_gelu(void* Y, const void* X, int64_t n, void* stream) {
  if (!Y || !X || n <= 0 || (((uintptr_t)Y | (uintptr_t)X) & 15)) { me_set_error("me_quick_gelu: bad arguments"); return ME_EINVAL; }
  (void)hipGetLastError();
  me_set_kernel("quick_gelu_kernel");
  hipLaunchKernelGGL(quick_gelu_kernel, dim3(grid_for((n + 7) / 8)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<f16*>(Y),
                     reinterpret_cast<const f16*>(X), (long)n);
  ME_CHECK_LAUNCH("me_quick_gelu")
}

extern "C" int me_attn_causal(void* O, int32_t ldo, const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, int32_t n_seq, int32_t heads,
                              int32_t dh, int32_t nq, float scale, void* stream) {
  if (!O || !Q || !K || !V || n_seq <= 0 || heads <= 0 || nq <= 0 || !(scale > 0.f)) { me_set_error("me_attn_causal: bad arguments"); return ME_EINVAL; }
  if (dh != CA_DH || nq > CA_MAXN) { me_set_error("me_attn_causal: serves dh = 64 and nq = nk <= 128 only"); return ME_EINVAL; }
  if ((ldo | ldq | ldk | ldv) % 8 || ldo < heads * dh || ldq < heads * dh || ldk < heads * dh || ldv < heads * dh ||
      (((uintptr_t)O | (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) || (int64_t)n_seq * heads > 0x7fffffff) {
    me_set_error("me_attn_causal: row strides must be multiples of 8 elements >= heads * dh, pointers 16-byte aligned");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  me_set_kernel("attn_causal_kernel");
  hipLaunchKernelGGL(attn_causal_kernel, dim3((unsigned)(n_seq * heads), (unsigned)((nq + CA_QB - 1) / CA_QB)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     reinterpret_cast<f16*>(O), ldo, reinterpret_cast<const f16*>(Q), ldq, reinterpret_cast<const f16*>(K), ldk, reinterpret_cast<const f16*>(V), ldv,
                     heads, nq, scale * 1.4426950408889634f);
  ME_CHECK_LAUNCH("me_attn_causal")
}
