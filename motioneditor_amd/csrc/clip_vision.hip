// CLIP vision tower and CLIP-metric kernels of libmotioned (gfx950): what transformers' CLIPVisionModelWithProjection and CLIPImageProcessor need beyond
// me_gemm / me_layernorm / me_quick_gelu, and the cosine the CLIP metrics are made of.
//   me_attn_full       bidirectional self-attention at head size 64 over 1 .. 288 tokens (50 / 197 / 257 in the ViT-B/32, B/16, L/14 towers)
//   me_patch_rows      fp32 pixel_values [n, 3, S, S] -> fp16 rows [n g^2, Kpad], the im2col of the stride = kernel patch convolution
//   me_vit_tokens      class token + patch rows + position embedding -> the token rows
//   me_resample_u8     one axis of PIL's antialiased resampling in its integer form (uint8 in, uint8 out, 22-bit coefficients from the host)
//   me_crop_normalize  centre crop + (u8 / 255 - mean) / std -> fp32 NCHW
//   me_cosine_rows     out[r] = a_r . b_r / (|a_r| |b_r|), fp32
// No atomics, every output element is written by exactly one thread: results are bitwise reproducible.
// The file takes the library's default flags (-ffp-contract=fast).  The normalisation must be three separately rounded fp32 operations, as numpy computes it:
// a division, a subtraction and a division hold no multiply-add to contract, and crop_normalize_kernel switches contraction off in its body besides.
#include "me_common.h"
#include "../../include/motioned_vision.h"

namespace {

// Bidirectional self-attention, dh = 64, nq = nk = n <= 288.  The form of attn_causal_kernel (csrc/clip.hip) without the mask and with the keys in dynamic
// LDS: block = (sequence, head, 64-query block), 4 waves, one 16-query tile per wave.  The block stages ALL keys of its (sequence, head): K row-major
// (pitch 72), V transposed (pitch npad + 8), npad = n rounded up to 32, zero-filled beyond n.  Every wave computes S^T = K Q^T per 16-key tile, so that the
// accumulator layout (lane l, register r: key (l >> 4) * 4 + r, query l & 15) is already the B-operand layout of O^T = V^T P^T once two key tiles are paired
// into one 32-deep contraction.  Softmax in fp32 over all keys at once (at most 18 tiles x 4 registers), row maximum subtracted; a key >= n (the tile
// padding: 257 = 16 * 16 + 1 leaves 15 of them in tile 16 and all of tile 17) gets weight exactly 0 and is left out of the denominator.
constexpr int FA_DH = 64, FA_NMAX = ME_ATTN_FULL_NMAX, FA_QB = 64, FA_KP = FA_DH + 8, FA_TILES = FA_NMAX / 16;
static_assert(FA_NMAX % 32 == 0, "paired key tiles");

inline size_t fa_lds_bytes(int n) {
  const int npad = (n + 31) & ~31;
  return (size_t)npad * FA_KP * sizeof(f16) + (size_t)FA_DH * (npad + 8) * sizeof(f16);
}

__global__ __launch_bounds__(256) void attn_full_kernel(f16* __restrict__ O, int ldo, const f16* __restrict__ Q, int ldq, const f16* __restrict__ K, int ldk,
                                                        const f16* __restrict__ V, int ldv, int heads, int n, float scale_log2e) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fa_smem[];
  const int npad = (n + 31) & ~31;                  // what the paired key tiles may touch: zero-filled beyond n
  const int vp = npad + 8;
  f16* Ks = reinterpret_cast<f16*>(fa_smem);        // [key][d], pitch 72
  f16* Vt = Ks + npad * FA_KP;                      // [d][key], pitch npad + 8
  const int seq = blockIdx.x / heads, head = blockIdx.x % heads;
  const long row0 = (long)seq * n;
  const int col0 = head * FA_DH;
  const int qb0 = blockIdx.y * FA_QB;
  const int tid = threadIdx.x;

  for (int i = tid; i < npad * (FA_DH / 8); i += 256) {
    const int key = i >> 3, c = (i & 7) << 3;
    U128 k, v;
    k.u = zero128();
    v.u = zero128();
    if (key < n) {
      k.u = ldg128(K + (row0 + key) * ldk + col0 + c);
      v.u = ldg128(V + (row0 + key) * ldv + col0 + c);
    }
    *reinterpret_cast<uint4*>(&Ks[key * FA_KP + c]) = k.u;
#pragma unroll
    for (int e = 0; e < 8; ++e) Vt[(c + e) * vp + key] = v.e[e];
  }
  __syncthreads();

  const int wave = tid >> 6, l = tid & 63;
  const int q0 = qb0 + wave * 16;
  if (q0 >= n) return;                               // (after the only barrier)
  const int li = l & 15, lg = l >> 4;
  const int q = q0 + li;
  const int nt = (n + 15) >> 4;                      // 16-key tiles that hold a key

  // Q^T as the B operand: lane holds Q[q][kk * 32 + lg * 8 + 0..7]; a padded query row reads as zeros and is not stored
  U128 qf[2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) {
    qf[kk].u = zero128();
    if (q < n) qf[kk].u = ldg128(Q + (row0 + q) * ldq + col0 + kk * 32 + lg * 8);
  }

  float s[FA_TILES][4];
  float m = -3.0e38f;
#pragma unroll
  for (int t = 0; t < FA_TILES; ++t) {
    if (t < nt) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        U128 a;
        a.u = *reinterpret_cast<const uint4*>(&Ks[(t * 16 + li) * FA_KP + kk * 32 + lg * 8]);
        acc = mfma16(a.h, qf[kk].h, acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const bool ok = t * 16 + lg * 4 + r < n;
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
  f16 p[FA_TILES][4];
#pragma unroll
  for (int t = 0; t < FA_TILES; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = t < nt && t * 16 + lg * 4 + r < n;
      const float e = ok ? __builtin_amdgcn_exp2f((s[t][r] - m) * scale_log2e) : 0.f;
      sum += e;
      p[t][r] = (f16)e;
    }
  }
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;    // the key of the row maximum weighs 1: sum >= 1

  // O^T[d][q] = sum_key V^T[d][key] P^T[key][q], key tiles in pairs (the second tile of the last pair may be all padding: zeros in LDS, weights 0)
  f32x4 o[FA_DH / 16];
#pragma unroll
  for (int dt = 0; dt < FA_DH / 16; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < FA_TILES / 2; ++j) {
    if (2 * j < nt) {
      f16x8 b;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        b[r] = p[2 * j][r];
        b[4 + r] = p[2 * j + 1][r];
      }
#pragma unroll
      for (int dt = 0; dt < FA_DH / 16; ++dt) {
        const f16* vrow = &Vt[(dt * 16 + li) * vp + lg * 4];
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
  if (q < n) {
#pragma unroll
    for (int dt = 0; dt < FA_DH / 16; ++dt) {   // lane l, register r: O[q][dt * 16 + lg * 4 + r]
      U64 w;
#pragma unroll
      for (int r = 0; r < 4; ++r) w.e[r] = (f16)(o[dt][r] * inv);
      *reinterpret_cast<uint2*>(O + (row0 + q) * ldo + col0 + dt * 16 + lg * 4) = w.u;
    }
  }
}

// out[(img * g + gy) * g + gx][(c * patch + py) * patch + px] = fp16(pix[img][c][gy * patch + py][gx * patch + px]); columns K .. Kpad - 1 are zeros.
// One thread = 8 columns of one row (one 16-byte store).
__global__ __launch_bounds__(256) void patch_rows_kernel(f16* __restrict__ out, int ldo, const float* __restrict__ pix, long s_img, long s_ch, int s_row, long rows, int g,
                                                         int patch, int K, int Kpad) {
  const int vec_per_row = Kpad >> 3;
  const long total = rows * vec_per_row;
  const int pp = patch * patch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / vec_per_row;
    const int c0 = (int)(idx - r * vec_per_row) << 3;
    const long img = r / (g * g);
    const int cell = (int)(r - img * (g * g));
    const int gy = cell / g, gx = cell - gy * g;
    const float* base = pix + img * s_img + (long)(gy * patch) * s_row + gx * patch;
    U128 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int col = c0 + e;
      float v = 0.f;
      if (col < K) {
        const int c = col / pp, rem = col - c * pp;
        const int py = rem / patch, px = rem - py * patch;
        v = base[c * s_ch + (long)py * s_row + px];
      }
      o.e[e] = (f16)v;
    }
    *reinterpret_cast<uint4*>(out + r * ldo + c0) = o.u;
  }
}

// x[i * T + 0] = fp16(cls + pos[0]); x[i * T + 1 + p] = fp16(patch_out[i * g2 + p] + pos[1 + p]), T = g2 + 1; fp32 sum rounded once; one thread = 8 columns.
__global__ __launch_bounds__(256) void vit_tokens_kernel(f16* __restrict__ x, int ldx, const f16* __restrict__ po, int ldp, const f16* __restrict__ cls,
                                                         const f16* __restrict__ pos, long rows, int g2, int C) {
  const int vec_per_row = C >> 3;
  const long total = rows * vec_per_row;
  const int T = g2 + 1;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long r = idx / vec_per_row;
    const int c = (int)(idx - r * vec_per_row) << 3;
    const long img = r / T;
    const int t = (int)(r - img * T);
    U128 a, p, o;
    a.u = t == 0 ? ldg128(cls + c) : ldg128(po + (img * g2 + t - 1) * ldp + c);
    p.u = ldg128(pos + (long)t * C + c);
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = (f16)((float)a.e[e] + (float)p.e[e]);
    *reinterpret_cast<uint4*>(x + r * ldx + c) = o.u;
  }
}

// One axis of PIL's ImagingResample (8 bits per channel): out = clip8((sum_k coef[o][k] * in[first[o] + k] + 2^21) >> 22), int32, arithmetic shift.
// bounds[2 o] = first input index, bounds[2 o + 1] = number of taps (<= ksize); AXIS 0: along x (out [n, H, out_size, C]), 1: along y (out [n, out_size, W, C]).
// One thread = one output pixel, all C channels.  A tap outside [0, size) -- no table of the wrapper has one -- is skipped, so a wrong table cannot make the
// kernel leave the image.
template <int C, int AXIS>
__global__ __launch_bounds__(256) void resample_u8_kernel(uint8_t* __restrict__ out, long o_img, int o_row, const uint8_t* __restrict__ src, long s_img, int s_row, int n,
                                                          int H, int W, int osz, const int* __restrict__ bounds, const int* __restrict__ coef, int ksize) {
  const int oh = AXIS ? osz : H, ow = AXIS ? W : osz;
  const long total = (long)n * oh * ow;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int ox = (int)(idx % ow);
    const long r = idx / ow;
    const int oy = (int)(r % oh);
    const long img = r / oh;
    const int o = AXIS ? oy : ox;
    const int first = bounds[2 * o], cnt = min(bounds[2 * o + 1], ksize);
    const int* ck = coef + (long)o * ksize;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
    const uint8_t* s = src + img * s_img;
    for (int k = 0; k < cnt; ++k) {
      const int i = first + k;
      if (i < 0 || i >= (AXIS ? H : W)) continue;
      const uint8_t* px = AXIS ? s + (long)i * s_row + ox * C : s + (long)oy * s_row + i * C;
      const int w = ck[k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += w * (int)px[c];
    }
    uint8_t* d = out + img * o_img + (long)oy * o_row + ox * C;
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = (uint8_t)min(max(acc[c] >> 22, 0), 255);
  }
}

// out[img][c][y][x] = ((float)src[img][top + y][left + x][c] / 255.0f - mean[c]) / std[c]: three separately rounded fp32 operations (numpy's, in
// CLIPImageProcessor: rescale by 1 / 255 as a division, then normalise).  One thread = one pixel, three channels.
__global__ __launch_bounds__(256) void crop_normalize_kernel(float* __restrict__ out, long o_img, long o_ch, int o_row, const uint8_t* __restrict__ src, long s_img,
                                                             int s_row, int n, int top, int left, int ch, int cw, float m0, float m1, float m2, float d0, float d1,
                                                             float d2) {
  const long total = (long)n * ch * cw;
  const float mean[3] = {m0, m1, m2}, sd[3] = {d0, d1, d2};
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int x = (int)(idx % cw);
    const long r = idx / cw;
    const int y = (int)(r % ch);
    const long img = r / ch;
    const uint8_t* px = src + img * s_img + (long)(top + y) * s_row + (left + x) * 3;
    float* o = out + img * o_img + (long)y * o_row + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma clang fp contract(off)
      const float v = (float)px[c] / 255.0f;
      const float w = v - mean[c];
      o[c * o_ch] = w / sd[c];
    }
  }
}

// out[r] = a_r . b_r / (sqrt(a_r . a_r) sqrt(b_r . b_r)); one wave per row, lane l sums columns l, l + 64, ... in ascending order, then the xor butterfly:
// a fixed order whatever the grid.  ldb == 0: every row is compared with the one row b.
__global__ __launch_bounds__(256) void cosine_rows_kernel(float* __restrict__ out, const float* __restrict__ a, long lda, const float* __restrict__ b, long ldb, long rows,
                                                          int C) {
  const int l = threadIdx.x & 63;
  for (long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (long)gridDim.x * 4) {
    const float* ar = a + r * lda;
    const float* br = b + r * ldb;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int c = l; c < C; c += 64) {
      const float x = ar[c], y = br[c];
      ab = __builtin_fmaf(x, y, ab);
      aa = __builtin_fmaf(x, x, aa);
      bb = __builtin_fmaf(y, y, bb);
    }
    ab = wave_sum(ab);
    aa = wave_sum(aa);
    bb = wave_sum(bb);
    if (l == 0) out[r] = ab / (sqrtf(aa) * sqrtf(bb));
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

extern "C" int me_attn_full_nmax(void) { return FA_NMAX; }

extern "C" int me_attn_full(void* O, int32_t ldo, const void* Q, int32_t ldq, const void* K, int32_t ldk, const void* V, int32_t ldv, int32_t n_seq, int32_t heads,
                            int32_t dh, int32_t n, float scale, void* stream) {
  if (!O || !Q || !K || !V || n_seq <= 0 || heads <= 0 || n <= 0 || !(scale > 0.f)) { me_set_error("me_attn_full: bad arguments"); return ME_EINVAL; }
  if (dh != FA_DH || n > FA_NMAX) { me_set_error("me_attn_full: serves dh = 64 and nq = nk <= 288 only"); return ME_EINVAL; }
  if ((ldo | ldq | ldk | ldv) % 8 || ldo < heads * dh || ldq < heads * dh || ldk < heads * dh || ldv < heads * dh ||
      (((uintptr_t)O | (uintptr_t)Q | (uintptr_t)K | (uintptr_t)V) & 15) || (int64_t)n_seq * heads > 0x7fffffff) {
    me_set_error("me_attn_full: row strides must be multiples of 8 elements >= heads * dh, pointers 16-byte aligned");
    return ME_EINVAL;
  }
  static bool attr_set_dev[64] = {};
  int dev_id = 0;
  (void)hipGetDevice(&dev_id);
  if (!attr_set_dev[dev_id & 63]) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_full_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)fa_lds_bytes(FA_NMAX)) != hipSuccess) {
      me_set_error("me_attn_full: hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      return ME_EHIP;
    }
    attr_set_dev[dev_id & 63] = true;
  }
  (void)hipGetLastError();  // drop stale errors left by other HIP users in this thread
  me_set_kernel("attn_full_kernel");
  hipLaunchKernelGGL(attn_full_kernel, dim3((unsigned)(n_seq * heads), (unsigned)((n + FA_QB - 1) / FA_QB)), dim3(256), fa_lds_bytes(n),
                     reinterpret_cast<hipStream_t>(stream), reinterpret_cast<f16*>(O), ldo, reinterpret_cast<const f16*>(Q), ldq, reinterpret_cast<const f16*>(K), ldk,
                     reinterpret_cast<const f16*>(V), ldv, heads, n, scale * 1.4426950408889634f);
  ME_CHECK_LAUNCH("me_attn_full")
}

extern "C" int me_patch_rows(void* out, int32_t ldo, const float* pix, int64_t img_stride, int64_t ch_stride, int32_t row_stride, int32_t n, int32_t S, int32_t patch,
                             void* stream) {
  if (!out || !pix || n <= 0 || S <= 0 || patch <= 0 || S % patch) { me_set_error("me_patch_rows: bad arguments (S a positive multiple of patch)"); return ME_EINVAL; }
  const int64_t K = 3LL * patch * patch, Kpad = (K + 7) & ~7LL;
  const int g = S / patch;
  if (Kpad > 0x7fffffff || ldo % 8 || ldo < Kpad || ((uintptr_t)out & 15) || ((uintptr_t)pix & 3) || S > row_stride || (int64_t)S * row_stride > ch_stride ||
      3 * ch_stride > img_stride) {
    me_set_error("me_patch_rows: out 16-byte aligned with a row stride that is a multiple of 8 >= Kpad; pix 4-byte aligned, strides (in elements) that keep rows, "
                 "channels and images apart");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  me_set_kernel("patch_rows_kernel");
  const long rows = (long)n * g * g;
  hipLaunchKernelGGL(patch_rows_kernel, dim3(grid_for(rows * (Kpad / 8))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<f16*>(out), ldo, pix,
                     (long)img_stride, (long)ch_stride, row_stride, rows, g, patch, (int)K, (int)Kpad);
  ME_CHECK_LAUNCH("me_patch_rows")
}

extern "C" int me_vit_tokens(void* x, int32_t ldx, const void* patch_out, int32_t ldp, const void* cls, const void* pos, int32_t n, int32_t g2, int32_t C, void* stream) {
  if (!x || !patch_out || !cls || !pos || n <= 0 || g2 <= 0 || C <= 0 || C % 8 || ldx % 8 || ldp % 8 || ldx < C || ldp < C ||
      (((uintptr_t)x | (uintptr_t)patch_out | (uintptr_t)cls | (uintptr_t)pos) & 15)) {
    me_set_error("me_vit_tokens: bad arguments (C and the row strides multiples of 8, strides >= C, 16-byte aligned pointers)");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  me_set_kernel("vit_tokens_kernel");
  const long rows = (long)n * (g2 + 1);
  hipLaunchKernelGGL(vit_tokens_kernel, dim3(grid_for(rows * (C / 8))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<f16*>(x), ldx,
                     reinterpret_cast<const f16*>(patch_out), ldp, reinterpret_cast<const f16*>(cls), reinterpret_cast<const f16*>(pos), rows, g2, C);
  ME_CHECK_LAUNCH("me_vit_tokens")
}

extern "C" int me_resample_u8(uint8_t* out, int64_t out_img_stride, int32_t out_row_stride, const uint8_t* src, int64_t src_img_stride, int32_t src_row_stride, int32_t n,
                              int32_t H, int32_t W, int32_t C, int32_t out_size, int32_t axis, const int32_t* bounds, const int32_t* coef, int32_t ksize, void* stream) {
  if (!out || !src || !bounds || !coef) { me_set_error("me_resample_u8: null pointer"); return ME_EINVAL; }
  if (C != 1 && C != 3) { me_set_error("me_resample_u8: C must be 1 or 3"); return ME_EINVAL; }
  if (axis != 0 && axis != 1) { me_set_error("me_resample_u8: axis must be 0 (along x) or 1 (along y)"); return ME_EINVAL; }
  if (n <= 0 || H <= 0 || W <= 0 || out_size <= 0 || ksize <= 0) { me_set_error("me_resample_u8: n, H, W, out_size, ksize must be positive"); return ME_EINVAL; }
  const int64_t oh = axis ? out_size : H, ow = axis ? W : out_size;
  if ((int64_t)W * C > src_row_stride || (int64_t)H * src_row_stride > src_img_stride || ow * C > out_row_stride || oh * out_row_stride > out_img_stride ||
      (((uintptr_t)bounds | (uintptr_t)coef) & 3)) {
    me_set_error("me_resample_u8: strides (in elements) must hold a row inside a row stride and the rows inside an image stride; tables 4-byte aligned");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  const dim3 grid(grid_for((long)n * oh * ow)), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define ME_RESAMPLE_LAUNCH(CC, AX)                                                                                                                          \
  hipLaunchKernelGGL((resample_u8_kernel<CC, AX>), grid, block, 0, st, out, (long)out_img_stride, out_row_stride, src, (long)src_img_stride, src_row_stride, n, H, W, \
                     out_size, reinterpret_cast<const int*>(bounds), reinterpret_cast<const int*>(coef), ksize)
  if (axis == 0) {
    me_set_kernel(C == 3 ? "resample_u8_kernel<3,x>" : "resample_u8_kernel<1,x>");
    if (C == 3) ME_RESAMPLE_LAUNCH(3, 0); else ME_RESAMPLE_LAUNCH(1, 0);
  } else {
    me_set_kernel(C == 3 ? "resample_u8_kernel<3,y>" : "resample_u8_kernel<1,y>");
    if (C == 3) ME_RESAMPLE_LAUNCH(3, 1); else ME_RESAMPLE_LAUNCH(1, 1);
  }
#undef ME_RESAMPLE_LAUNCH
  ME_CHECK_LAUNCH("me_resample_u8")
}

extern "C" int me_crop_normalize(float* out, int64_t out_img_stride, int64_t out_ch_stride, int32_t out_row_stride, const uint8_t* src, int64_t src_img_stride,
                                 int32_t src_row_stride, int32_t n, int32_t H, int32_t W, int32_t top, int32_t left, int32_t crop_h, int32_t crop_w, float mean0,
                                 float mean1, float mean2, float std0, float std1, float std2, void* stream) {
  if (!out || !src) { me_set_error("me_crop_normalize: null pointer"); return ME_EINVAL; }
  if (n <= 0 || H <= 0 || W <= 0 || crop_h <= 0 || crop_w <= 0 || top < 0 || left < 0 || (int64_t)top + crop_h > H || (int64_t)left + crop_w > W) {
    me_set_error("me_crop_normalize: the crop window must lie inside the image");
    return ME_EINVAL;
  }
  if ((int64_t)W * 3 > src_row_stride || (int64_t)H * src_row_stride > src_img_stride || crop_w > out_row_stride || (int64_t)crop_h * out_row_stride > out_ch_stride ||
      3 * out_ch_stride > out_img_stride || ((uintptr_t)out & 3)) {
    me_set_error("me_crop_normalize: strides (in elements) must hold a row inside a row stride, the rows inside a channel / image stride; out 4-byte aligned");
    return ME_EINVAL;
  }
  if (!(std0 != 0.f) || !(std1 != 0.f) || !(std2 != 0.f) || std0 != std0 || std1 != std1 || std2 != std2 || mean0 != mean0 || mean1 != mean1 || mean2 != mean2) {
    me_set_error("me_crop_normalize: every std must be a non-zero number, every mean a number");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  me_set_kernel("crop_normalize_kernel");
  hipLaunchKernelGGL(crop_normalize_kernel, dim3(grid_for((long)n * crop_h * crop_w)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, (long)out_img_stride,
                     (long)out_ch_stride, out_row_stride, src, (long)src_img_stride, src_row_stride, n, top, left, crop_h, crop_w, mean0, mean1, mean2, std0, std1, std2);
  ME_CHECK_LAUNCH("me_crop_normalize")
}

extern "C" int me_cosine_rows(float* out, const float* a, int64_t lda, const float* b, int64_t ldb, int64_t rows, int32_t C, void* stream) {
  if (!out || !a || !b || rows <= 0 || C <= 0 || lda < C || (ldb != 0 && ldb < C) || (((uintptr_t)out | (uintptr_t)a | (uintptr_t)b) & 3)) {
    me_set_error("me_cosine_rows: bad arguments (lda >= C; ldb >= C, or 0 for one shared row; 4-byte aligned pointers)");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  me_set_kernel("cosine_rows_kernel");
  long blocks = (rows + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  hipLaunchKernelGGL(cosine_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, a, (long)lda, b, (long)ldb, (long)rows, C);
  ME_CHECK_LAUNCH("me_cosine_rows")
}
