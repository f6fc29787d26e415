// Stage-1 tuning beyond the dense projections (gfx950): the weight gradient of the 3x3 convolutions in one call (me_conv_dw), the GroupNorm
// affine gradients (me_groupnorm_bwd_params) and the in-place refresh of the folded upsampler weight (me_refresh_ups4) -- the device side of
// train_bg.py's trainable_modules for ResnetBlock2D / Downsample2D / Upsample2D / GroupNorm.  include/motioned_tune.h states the contracts.
// Deterministic like csrc/train.hip: reductions over the row axis go through fixed-order fp32 partials, never atomics.
#include "me_common.h"
#include "../../include/motioned_tune.h"

extern "C" void me_set_error(const char* msg);
extern "C" void me_set_hip_error(const char* what, int err);
extern "C" void me_set_kernel(const char* name);

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// 3x3 weight gradient: work[s][n][tap][k] = sum over the split's rows m of dY[m, n] * X[src(m, tap), k]   (fp32, MFMA)
// Block tile 64 (k) x 64 (n) x nine taps, 4 waves of 32 x 32 x 9: 36 accumulator tiles = 144 registers per lane.  A row stage is 32 output rows: the
// dY tile is staged ONCE and multiplied with the nine gathered X tiles (gemm_dw_kernel nine times stages it nine times).  All ten tiles lie
// ROW-major in LDS ([row][column], written with 16-byte stores as they arrive from memory); both MFMA operands are contracted over the row index
// and come out of ds_read_b64_tr_b16, which hands a lane one column of four rows -- no 2-byte transposing stores.
//   MFMA k-slot (g, j) = stage row 4 g + j (j < 4), 16 + 4 g + (j - 4) (j >= 4), for A and B alike: the half-wave's two lane groups then read eight
//   consecutive rows, which the 160-byte row pitch spreads over all 64 banks.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int CW_MS = 32;            // rows per stage
constexpr int CW_LD = 64 + 16;       // f16 per LDS row: 160 bytes (16-byte aligned rows; rows r .. r + 7 start on distinct 8-bank slots)
constexpr int CW_TILE = CW_MS * CW_LD;

typedef __fp16 h16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));

// column c0 + (lane & 15) of stage rows (g, 0..7) of a row-major tile, as the 8 k-slots of one MFMA operand
__device__ __forceinline__ f16x8 cw_operand(const f16* tile, int c0, int lane) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const f16* p0 = tile + (4 * g + q) * CW_LD + c0 + 4 * p;   // this lane's ADDRESS: row q of the group's 4 x 16 block, columns 4 p .. 4 p + 3
  const h16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h16x4*)(p0));
  const h16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) h16x4*)(p0 + 16 * CW_LD));
  const f16x4 l4 = __builtin_bit_cast(f16x4, lo), h4 = __builtin_bit_cast(f16x4, hi);
  return f16x8{l4[0], l4[1], l4[2], l4[3], h4[0], h4[1], h4[2], h4[3]};
}

template <int DYF16>
__global__ __launch_bounds__(256) void conv_dw_kernel(const me_conv_dw_args a, int splits, int rows_per_split) {
  __shared__ __attribute__((aligned(16))) f16 sT[10 * CW_TILE];   // tile 0: dY [row][n]; tile 1 + tap: X rows of the tap [row][k]
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, l15 = lane & 15;
  const int wk = wave >> 1, wn = wave & 1;

  const int nbk = (a.K + 63) / 64, nbn = (a.N + 63) / 64;
  int w = blockIdx.x;
  const int bk = w % nbk;
  w /= nbk;
  const int bn = w % nbn;
  const int sp = w / nbn;
  const int k0 = bk * 64, n0 = bn * 64;
  const long m0 = (long)sp * rows_per_split;
  const long m1 = m0 + rows_per_split < a.M ? m0 + rows_per_split : a.M;

  const f16* __restrict__ X = reinterpret_cast<const f16*>(a.X);
  f32x4 acc[9][2][2];   // [tap][k tile][n tile]
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[t][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging map: thread -> (row r = tid / 8, 8-column chunk cc = tid % 8) of every 32 x 64 tile
  const int r = tid >> 3, cc = tid & 7;
  const bool kok = k0 + cc * 8 < a.K, nok = n0 + cc * 8 < a.N;
  const int hw = a.Hout * a.Wout;
  const int Hv = a.Hin << a.ups, Wv = a.Win << a.ups;
  f16* const srow = sT + r * CW_LD + cc * 8;
  for (long mb = m0; mb < m1; mb += CW_MS) {
    const long m = mb + r;
    const bool mok = m < m1;
    // the forward's ME_GATHER_CONV3 row: image, output pixel, top-left virtual pixel of its 3 x 3 window
    const int img = (int)(m / hw);
    const int rem = (int)(m - (long)img * hw);
    const int oy = rem / a.Wout, ox = rem - oy * a.Wout;
    const long base = (long)img * a.Hin * a.Win;
    const int y0 = oy * a.stride - 1, x0 = ox * a.stride - 1;
    uint4 ux[9], ud;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = y0 + t / 3, ix = x0 + t % 3;
      const bool ok = mok && kok && iy >= 0 && iy < Hv && ix >= 0 && ix < Wv;   // outside the image: a zero row, never the neighbouring row / image
      ux[t] = ok ? ldg128(X + (base + (long)(iy >> a.ups) * a.Win + (ix >> a.ups)) * a.ldx + k0 + cc * 8) : zero128();
    }
    if (mok && nok) {
      if (DYF16) {
        ud = ldg128(reinterpret_cast<const f16*>(a.dY) + m * a.lddy + n0 + cc * 8);
      } else {
        const float* p = reinterpret_cast<const float*>(a.dY) + m * a.lddy + n0 + cc * 8;
        const float4 f0 = *reinterpret_cast<const float4*>(p), f1 = *reinterpret_cast<const float4*>(p + 4);
        U128 u;
        u.e[0] = (f16)f0.x; u.e[1] = (f16)f0.y; u.e[2] = (f16)f0.z; u.e[3] = (f16)f0.w;
        u.e[4] = (f16)f1.x; u.e[5] = (f16)f1.y; u.e[6] = (f16)f1.z; u.e[7] = (f16)f1.w;
        ud = u.u;
      }
    } else {
      ud = zero128();
    }
    *reinterpret_cast<uint4*>(srow) = ud;
#pragma unroll
    for (int t = 0; t < 9; ++t) *reinterpret_cast<uint4*>(srow + (1 + t) * CW_TILE) = ux[t];
    __syncthreads();
    // every lane of every wave reads (the transposing read needs the whole wave: no lane-dependent control flow from here to the barrier)
    f16x8 fb[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) fb[j] = cw_operand(sT, wn * 32 + j * 16, lane);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      f16x8 fa[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = cw_operand(sT + (1 + t) * CW_TILE, wk * 32 + i * 16, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[t][i][j] = mfma16(fa[i], fb[j], acc[t][i][j]);
    }
    __syncthreads();
  }
  // D[i = k][n' = n]: lane (n = l15, g), reg r <-> k = g * 4 + r
  float* work = reinterpret_cast<float*>(a.work) + (long)sp * a.N * 9 * a.K;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int k = k0 + wk * 32 + i * 16 + g * 4, n = n0 + wn * 32 + j * 16 + l15;
        if (n < a.N && k < a.K)
          *reinterpret_cast<float4*>(work + ((long)n * 9 + t) * a.K + k) = make_float4(acc[t][i][j][0], acc[t][i][j][1], acc[t][i][j][2], acc[t][i][j][3]);
      }
}

// dW[i] += alpha * sum_s work[s][i] over the whole [N][9][K] tensor, splits added in index order (4 elements per thread)
__global__ __launch_bounds__(256) void conv_dw_fold_kernel(const float* __restrict__ work, float* dW, long total, int splits, float alpha) {
  for (long idx = ((long)blockIdx.x * 256 + threadIdx.x) * 4; idx < total; idx += (long)gridDim.x * 1024) {
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int sp = 0; sp < splits; ++sp) {
      const float4 v = *reinterpret_cast<const float4*>(work + (long)sp * total + idx);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    float4 o = *reinterpret_cast<float4*>(dW + idx);
    o.x += alpha * s.x; o.y += alpha * s.y; o.z += alpha * s.z; o.w += alpha * s.w;
    *reinterpret_cast<float4*>(dW + idx) = o;
  }
}

constexpr int64_t CW_WORK_CAP = 256ll << 20;

void cw_geometry(int M, int N, int K, int* splits, int* rows_per_split) {
  const long tiles = (long)((N + 63) / 64) * ((K + 63) / 64);
  long s = (1024 + tiles - 1) / tiles;                         // ~1024 blocks
  const long smax = (M + 4 * CW_MS - 1) / (4 * CW_MS);         // at least four stages per split
  const long scap = CW_WORK_CAP / ((int64_t)N * 9 * K * (int64_t)sizeof(float));   // the partials stay inside 256 MiB
  if (s > smax) s = smax;
  if (s > scap) s = scap;
  if (s > 256) s = 256;
  if (s < 1) s = 1;
  long rps = (M + s - 1) / s;
  rps = (rps + CW_MS - 1) / CW_MS * CW_MS;
  s = (M + rps - 1) / rps;
  *splits = (int)s;
  *rows_per_split = (int)rps;
}

// ---------------------------------------------------------------------------------------------------------------------
// GroupNorm affine gradients: a thread owns one channel and walks down the rows of its block's row range (the statistics are the forward's
// deterministic fp64 sums, me_groupnorm_stats); row ranges are folded in index order
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gn_params_part_kernel(const f16* __restrict__ X, int ldx, const float* __restrict__ dY, int lddy, const f16* __restrict__ gamma,
                                                             const f16* __restrict__ beta, const double* __restrict__ stats, float* __restrict__ part, long rows,
                                                             int rows_per_group, int rows_per_block, int C, int groups, float eps, int silu) {
  const int c = blockIdx.y * 256 + threadIdx.x;
  if (c >= C) return;
  const long r0 = (long)blockIdx.x * rows_per_block, r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  const int cg = C / groups, ge = c / cg;
  const double inv_cnt = 1.0 / ((double)rows_per_group * (double)cg);
  const float gm = (float)gamma[c], bt = (float)beta[c];
  float sg_ = 0.f, sb_ = 0.f;
  long row = r0;
  while (row < r1) {
    const long sg = row / rows_per_group;
    const long seg_end = (sg + 1) * rows_per_group < r1 ? (sg + 1) * rows_per_group : r1;
    const double mean_d = stats[(sg * groups + ge) * 2 + 0] * inv_cnt;
    const float var = fmaxf((float)(stats[(sg * groups + ge) * 2 + 1] * inv_cnt - mean_d * mean_d), 0.f);
    const float mean = (float)mean_d, rstd = rsqrtf(var + eps);
    for (; row < seg_end; ++row) {
      const float xh = ((float)X[row * ldx + c] - mean) * rstd;
      float d = dY[row * lddy + c];
      if (silu) {
        const float y = __builtin_fmaf(xh, gm, bt);
        const float sig = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * y));
        d *= sig * (1.0f + y * (1.0f - sig));
      }
      sg_ += d * xh;
      sb_ += d;
    }
  }
  part[((long)blockIdx.x * 2 + 0) * C + c] = sg_;
  part[((long)blockIdx.x * 2 + 1) * C + c] = sb_;
}

__global__ __launch_bounds__(256) void gn_params_fold_kernel(const float* __restrict__ part, float* dgamma, float* dbeta, int C, int nparts, float alpha) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float sg = 0.f, sb = 0.f;
  for (int p = 0; p < nparts; ++p) {
    sg += part[((long)p * 2 + 0) * C + c];
    sb += part[((long)p * 2 + 1) * C + c];
  }
  if (dgamma) dgamma[c] += alpha * sg;
  if (dbeta) dbeta[c] += alpha * sb;
}

int gn_params_blocks(int64_t rows) {
  long b = (rows + 63) / 64;   // >= 64 rows per block
  if (b > 512) b = 512;
  if (b < 1) b = 1;
  return (int)b;
}

// ---------------------------------------------------------------------------------------------------------------------
// folded upsampler weight: dst[n][4 (2 py + px) + 2 ty + tx][k] = f16(sum of the 3x3 taps that fall on low-res pixel (ty, tx) of parity (py, px)),
// added in fp32 in (ky, kx) order from zero -- the additions of weights.Packed.fold_ups, one rounding
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void refresh_ups4_kernel(f16* __restrict__ dst, const float* __restrict__ master, int N, int K) {
  const int vpr = K / 4;
  const long total = (long)N * 16 * vpr;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int kv = (int)(idx % vpr);
    const long nt = idx / vpr;
    const int slot = (int)(nt & 15);
    const long n = nt >> 4;
    const int py = slot >> 3, px = (slot >> 2) & 1, ty = (slot >> 1) & 1, tx = slot & 1;
    f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx)
        if ((py + ky + 1) / 2 - py == ty && (px + kx + 1) / 2 - px == tx) s += *reinterpret_cast<const f32x4*>(master + (n * 9 + ky * 3 + kx) * K + kv * 4);
    *reinterpret_cast<f16x4*>(dst + nt * K + kv * 4) = f16x4{(f16)s[0], (f16)s[1], (f16)s[2], (f16)s[3]};
  }
}

inline unsigned grid_for(long n, long cap) {
  long b = (n + 255) / 256;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (unsigned)b;
}

}  // namespace

#define ME_TUNE_CHECK(name)                                                         \
  {                                                                                 \
    const hipError_t e_ = hipGetLastError();                                        \
    if (e_ != hipSuccess) { me_set_hip_error(name, (int)e_); return ME_EHIP; }      \
    return ME_OK;                                                                   \
  }

extern "C" int32_t me_conv_dw_splits(int32_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int s, rps;
  cw_geometry(M, N, K, &s, &rps);
  return s;
}

extern "C" int64_t me_conv_dw_work_bytes(int32_t M, int32_t N, int32_t K) {
  if (M <= 0 || N <= 0 || K <= 0) return 0;
  int s, rps;
  cw_geometry(M, N, K, &s, &rps);
  return (int64_t)s * N * 9 * K * (int64_t)sizeof(float);
}

extern "C" int me_conv_dw(const me_conv_dw_args* a, void* stream) {
  if (!a || !a->dY || !a->X || !a->dW || !a->work) { me_set_error("me_conv_dw: null pointer"); return ME_EINVAL; }
  if (a->M <= 0 || a->N <= 0 || a->K <= 0 || a->N % 8 || a->K % 8 || a->ldx % 8 || a->lddy % (a->dy_is_f16 ? 8 : 4) || a->ldx < a->K || a->lddy < a->N) {
    me_set_error("me_conv_dw: N, K, ldx must be multiples of 8, lddy of 4 (fp32) / 8 (fp16), and the strides cover K / N columns");
    return ME_EINVAL;
  }
  if (((uintptr_t)a->dY | (uintptr_t)a->X | (uintptr_t)a->dW | (uintptr_t)a->work) & 15) { me_set_error("me_conv_dw: misaligned pointer"); return ME_EINVAL; }
  if (a->pad0) { me_set_error("me_conv_dw: the pad-(0,1,0,1) convolution (pad0, the VAE encoder's form) is not differentiated"); return ME_EINVAL; }
  if (a->ups != 0 && a->ups != 1) { me_set_error("me_conv_dw: ups must be 0 or 1 (the zero-stuffed and the folded forms, ups 2 / 3, have no weight gradient)"); return ME_EINVAL; }
  if (a->stride != 1 && a->stride != 2) { me_set_error("me_conv_dw: stride must be 1 or 2"); return ME_EINVAL; }
  if (a->stride == 2 && a->ups) { me_set_error("me_conv_dw: stride 2 together with ups is not a convolution of the UNet"); return ME_EINVAL; }
  if (a->Hin <= 0 || a->Win <= 0 || a->Hout != ((a->Hin << a->ups) - 1) / a->stride + 1 || a->Wout != ((a->Win << a->ups) - 1) / a->stride + 1 ||
      a->M % (a->Hout * a->Wout)) {
    me_set_error("me_conv_dw: bad conv geometry (Hout = ((Hin << ups) - 1) / stride + 1, Wout alike, M whole images of Hout x Wout rows)");
    return ME_EINVAL;
  }
  if ((int64_t)a->N * 9 * a->K * (int64_t)sizeof(float) > CW_WORK_CAP) { me_set_error("me_conv_dw: N * 9 * K fp32 partials exceed the 256 MiB scratch"); return ME_EINVAL; }
  int splits, rps;
  cw_geometry(a->M, a->N, a->K, &splits, &rps);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  (void)hipGetLastError();
  const long blocks = (long)((a->K + 63) / 64) * ((a->N + 63) / 64) * splits;
  const long total = (long)a->N * 9 * a->K;
  if (a->dy_is_f16) {
    hipLaunchKernelGGL(conv_dw_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, st, *a, splits, rps);
    me_set_kernel("conv_dw_kernel<f16>");
  } else {
    hipLaunchKernelGGL(conv_dw_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, st, *a, splits, rps);
    me_set_kernel("conv_dw_kernel<f32>");
  }
  hipLaunchKernelGGL(conv_dw_fold_kernel, dim3(grid_for(total / 4, 4096)), dim3(256), 0, st, reinterpret_cast<const float*>(a->work), reinterpret_cast<float*>(a->dW), total,
                     splits, a->alpha);
  ME_TUNE_CHECK("me_conv_dw")
}

extern "C" int64_t me_groupnorm_bwd_params_work_bytes(int64_t rows, int32_t rows_per_group, int32_t C, int32_t groups) {
  if (rows <= 0 || rows > INT32_MAX || rows_per_group <= 0 || rows % rows_per_group || C <= 0 || groups <= 0) return 0;
  const int64_t fwd = (me_groupnorm_scratch_bytes((int32_t)rows, rows_per_group, groups) + 15) / 16 * 16;
  return fwd + (int64_t)gn_params_blocks(rows) * 2 * C * (int64_t)sizeof(float);
}

extern "C" int me_groupnorm_bwd_params(float* dgamma, float* dbeta, const void* x, int32_t ldx, const void* gamma, const void* beta, const void* dy, int32_t lddy,
                                       int64_t rows, int32_t rows_per_group, int32_t C, int32_t groups, float eps, int32_t silu, float alpha, void* work, void* stream) {
  if ((!dgamma && !dbeta) || !x || !gamma || !beta || !dy || !work || rows <= 0 || rows > INT32_MAX || rows_per_group <= 0 || rows % rows_per_group) {
    me_set_error("me_groupnorm_bwd_params: bad arguments (null pointer, or rows not a positive multiple of rows_per_group)");
    return ME_EINVAL;
  }
  if (groups <= 0 || groups > 64 || C <= 0 || C % groups || C % 8 || C > 2560) {
    me_set_error("me_groupnorm_bwd_params: bad channels (1 <= groups <= 64, C a multiple of groups and of 8, C <= 2560)");
    return ME_EINVAL;
  }
  if (ldx % 8 || lddy % 4 || ldx < C || lddy < C) { me_set_error("me_groupnorm_bwd_params: row strides must be multiples of 8 (x) / 4 (dy) and cover C columns"); return ME_EINVAL; }
  if ((((uintptr_t)x | (uintptr_t)dy | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)work) & 15) || (((uintptr_t)dgamma | (uintptr_t)dbeta) & 3)) {
    me_set_error("me_groupnorm_bwd_params: misaligned pointer");
    return ME_EINVAL;
  }
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  // statistics: the forward's deterministic pass
  me_groupnorm_args fa{};
  fa.X = x;
  fa.Y = const_cast<void*>(x);   // not written by the statistics pass
  fa.gamma = gamma;
  fa.beta = beta;
  fa.stats = work;
  fa.rows = (int32_t)rows;
  fa.rows_per_group = rows_per_group;
  fa.C = C;
  fa.ldx = ldx;
  fa.ldy = ldx;
  fa.groups = groups;
  fa.eps = eps;
  if (int rc = me_groupnorm_stats(&fa, stream)) return rc;
  const int64_t fwd = (me_groupnorm_scratch_bytes((int32_t)rows, rows_per_group, groups) + 15) / 16 * 16;
  float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(work) + fwd);
  const int nb = gn_params_blocks(rows);
  const int rpb = (int)((rows + nb - 1) / nb);
  (void)hipGetLastError();
  hipLaunchKernelGGL(gn_params_part_kernel, dim3((unsigned)nb, (unsigned)((C + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const f16*>(x), ldx,
                     reinterpret_cast<const float*>(dy), lddy, reinterpret_cast<const f16*>(gamma), reinterpret_cast<const f16*>(beta), reinterpret_cast<const double*>(work),
                     part, (long)rows, rows_per_group, rpb, C, groups, eps, silu);
  hipLaunchKernelGGL(gn_params_fold_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, part, dgamma, dbeta, C, nb, alpha);
  me_set_kernel("gn_params_part_kernel");
  ME_TUNE_CHECK("me_groupnorm_bwd_params")
}

extern "C" int me_refresh_ups4(void* dst, const float* master, int32_t N, int32_t K, void* stream) {
  if (!dst || !master || N <= 0 || K <= 0 || K % 4) { me_set_error("me_refresh_ups4: bad arguments (K a positive multiple of 4)"); return ME_EINVAL; }
  if (((uintptr_t)master & 15) || ((uintptr_t)dst & 7)) { me_set_error("me_refresh_ups4: misaligned pointer (master 16-byte, dst 8-byte aligned)"); return ME_EINVAL; }
  (void)hipGetLastError();
  hipLaunchKernelGGL(refresh_ups4_kernel, dim3(grid_for((long)N * 16 * (K / 4), 8192)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<f16*>(dst), master,
                     (int)N, (int)K);
  me_set_kernel("refresh_ups4_kernel");
  ME_TUNE_CHECK("me_refresh_ups4")
}
