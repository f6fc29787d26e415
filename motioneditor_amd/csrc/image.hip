// Clip I/O kernels of libmotioned (gfx950): the two places where the reference moves pixels between files and tensors.
//   me_image_resize   decoded uint8 HWC frames -> fp32 NCHW at the working size (F.interpolate bilinear / nearest, align_corners=False, no
//                     antialiasing) with the affine v / div + add folded in (motion_editor/data/dataset.py:121-144)
//   me_video_grid_u8  fp32 video [b, c, f, h, w] -> uint8 frames [f, Hg, Wg, 3]: torchvision.utils.make_grid per frame, (x + 1) / 2, * 255,
//                     uint8 (motion_editor/util.py:34-43)
// Both are HBM-bound copies with a gather; no atomics, every output element is written by exactly one thread, so results are bitwise reproducible.
// This file is compiled with -ffp-contract=off (build.EXTRA_FLAGS): the coordinate and weight expressions below are the separately rounded fp32
// operations of the torch kernels they restate, and a fused multiply-add would move a weight by an ulp of the coordinate.
#include "me_common.h"
#include "../../include/motioned_io.h"

namespace {

constexpr int PX = 4;   // output pixels along x per thread: one 16-byte fp32 store per channel (resize), three 4-byte stores (grid)

// area_pixel_compute_source_index(scale, dst, align_corners=False, cubic=False) of ATen, fp32
__device__ __forceinline__ void bilinear_coord(float scale, int dst, int size, int& i0, int& i1, float& w0, float& w1) {
  const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  i0 = min((int)src, size - 1);
  i1 = min(i0 + 1, size - 1);
  w1 = src - (float)i0;
  w0 = 1.0f - w1;
}
// nearest_idx of ATen, fp32
__device__ __forceinline__ int nearest_coord(float scale, int dst, int size) { return min((int)floorf((float)dst * scale), size - 1); }

// One thread: PX consecutive output pixels of one output row of one image, all C channels (the coordinates and the four taps are shared by the
// channels, whose bytes are neighbours in HWC).  Consecutive lanes hold consecutive pixel groups: per channel the wave stores 64 x 16 contiguous
// bytes.  A group that crosses the right edge, or whose address is not 16-byte aligned, stores its pixels one by one.
template <int C, int MODE>
__global__ __launch_bounds__(256) void image_resize_kernel(float* __restrict__ out, long o_img, long o_ch, int o_row, const uint8_t* __restrict__ src, long s_img,
                                                           int s_row, int n, int H, int W, int oh, int ow, float div, float add) {
  const int xg = (ow + PX - 1) / PX;
  const long total = (long)n * oh * xg;
  const float sy = (float)H / (float)oh, sx = (float)W / (float)ow;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx % xg);
    const long r = idx / xg;
    const int oy = (int)(r % oh);
    const long img = r / oh;
    const int x0 = g * PX;
    const uint8_t* s = src + img * s_img;
    float v[C][PX];
    if (MODE == ME_RESIZE_BILINEAR) {
      int y0, y1;
      float wy0, wy1;
      bilinear_coord(sy, oy, H, y0, y1, wy0, wy1);
      const uint8_t* r0 = s + (long)y0 * s_row;
      const uint8_t* r1 = s + (long)y1 * s_row;
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int ox = min(x0 + p, ow - 1);   // a lane past the right edge computes the last pixel again and does not store it
        int xa, xb;
        float wx0, wx1;
        bilinear_coord(sx, ox, W, xa, xb, wx0, wx1);
#pragma unroll
        for (int c = 0; c < C; ++c) {
          const float a = (float)r0[xa * C + c], b = (float)r0[xb * C + c], cc = (float)r1[xa * C + c], d = (float)r1[xb * C + c];
          v[c][p] = wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * cc + wx1 * d);
        }
      }
    } else {
      const uint8_t* r0 = s + (long)nearest_coord(sy, oy, H) * s_row;
#pragma unroll
      for (int p = 0; p < PX; ++p) {
        const int xa = nearest_coord(sx, min(x0 + p, ow - 1), W);
#pragma unroll
        for (int c = 0; c < C; ++c) v[c][p] = (float)r0[xa * C + c];
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float* o = out + img * o_img + c * o_ch + (long)oy * o_row + x0;
      f32x4 w;
#pragma unroll
      for (int p = 0; p < PX; ++p) w[p] = v[c][p] / div + add;
      if (x0 + PX <= ow && ((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<f32x4*>(o) = w;
      } else {
#pragma unroll
        for (int p = 0; p < PX; ++p)
          if (x0 + p < ow) o[p] = w[p];
      }
    }
  }
}

// (x + 1) / 2 when asked, * 255, clamped to [0, 255] (NaN -> 0), truncated
__device__ __forceinline__ unsigned to_u8(float x, int rescale) {
  if (rescale) x = (x + 1.0f) / 2.0f;
  x = x * 255.0f;
  x = fminf(fmaxf(x, 0.f), 255.f);
  return (unsigned)(int)x;
}

// One thread: PX consecutive pixels (12 bytes) of one row of one output frame.  pad = 0: the frame is the image (b == 1); pad = 2: make_grid's
// cells of (h + 2) x (w + 2) with image k = y * xmaps + x at rows y (h + 2) + 2, columns x (w + 2) + 2; every other pixel is the grid's 0.
__global__ __launch_bounds__(256) void video_grid_u8_kernel(uint8_t* __restrict__ out, long o_frame, int o_row, const float* __restrict__ vid, long s_b, long s_c,
                                                            long s_f, int s_row, int b, int c, int f, int h, int w, int xmaps, int pad, int Hg, int Wg, int rescale) {
  const int xg = (Wg + PX - 1) / PX;
  const long total = (long)f * Hg * xg;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int g = (int)(idx % xg);
    const long r = idx / xg;
    const int gy = (int)(r % Hg);
    const long t = r / Hg;
    const int x0 = g * PX;
    // the image row this grid row shows, if any
    int cy = 0, iy = gy;
    if (pad) {
      cy = gy / (h + pad);
      iy = gy - cy * (h + pad) - pad;
    }
    const bool row_in = iy >= 0 && iy < h;
    union {
      uint8_t e[PX * 3];
      uint32_t u[3];
    } px;
#pragma unroll
    for (int p = 0; p < PX; ++p) {
      const int gx = x0 + p;
      int cx = 0, ix = gx;
      if (pad) {
        cx = gx / (w + pad);
        ix = gx - cx * (w + pad) - pad;
      }
      const int k = cy * xmaps + cx;
      const bool in = row_in && gx < Wg && ix >= 0 && ix < w && cx < xmaps && k < b;
      float v[3] = {0.f, 0.f, 0.f};
      if (in) {
        const float* q = vid + k * s_b + t * s_f + (long)iy * s_row + ix;
        v[0] = q[0];
        v[1] = c == 3 ? q[s_c] : v[0];
        v[2] = c == 3 ? q[2 * s_c] : v[0];
      }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) px.e[p * 3 + ch] = (uint8_t)to_u8(v[ch], rescale);
    }
    uint8_t* o = out + t * o_frame + (long)gy * o_row + (long)x0 * 3;
    if (x0 + PX <= Wg && ((uintptr_t)o & 3) == 0) {
      uint32_t* o4 = reinterpret_cast<uint32_t*>(o);
      o4[0] = px.u[0];
      o4[1] = px.u[1];
      o4[2] = px.u[2];
    } else {
#pragma unroll
      for (int p = 0; p < PX; ++p)
        if (x0 + p < Wg) {
          o[p * 3 + 0] = px.e[p * 3 + 0];
          o[p * 3 + 1] = px.e[p * 3 + 1];
          o[p * 3 + 2] = px.e[p * 3 + 2];
        }
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

extern "C" int me_image_resize(float* out, int64_t out_img_stride, int64_t out_ch_stride, int32_t out_row_stride, const uint8_t* src, int64_t src_img_stride,
                               int32_t src_row_stride, int32_t n, int32_t H, int32_t W, int32_t C, int32_t oh, int32_t ow, int32_t mode, float div, float add,
                               void* stream) {
  if (!out || !src) { me_set_error("me_image_resize: null pointer"); return ME_EINVAL; }
  if (C != 1 && C != 3) { me_set_error("me_image_resize: C must be 1 or 3"); return ME_EINVAL; }
  if (n <= 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) { me_set_error("me_image_resize: n, H, W, oh, ow must be positive"); return ME_EINVAL; }
  if (mode != ME_RESIZE_BILINEAR && mode != ME_RESIZE_NEAREST) { me_set_error("me_image_resize: unknown mode (ME_RESIZE_BILINEAR = 0, ME_RESIZE_NEAREST = 1)"); return ME_EINVAL; }
  if ((int64_t)W * C > src_row_stride || (int64_t)H * src_row_stride > src_img_stride || ow > out_row_stride || (int64_t)oh * out_row_stride > out_ch_stride ||
      (int64_t)C * out_ch_stride > out_img_stride || ((uintptr_t)out & 3)) {
    me_set_error("me_image_resize: strides (in elements) must hold a row inside a row stride, the rows inside a channel / image stride; out 4-byte aligned");
    return ME_EINVAL;
  }
  if (!(div != 0.f) || div != div || add != add) { me_set_error("me_image_resize: div must be a non-zero number, add a number"); return ME_EINVAL; }
  (void)hipGetLastError();  // drop stale errors left by other HIP users in this thread
  const dim3 grid(grid_for((long)n * oh * ((ow + PX - 1) / PX))), block(256);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#define ME_RESIZE_LAUNCH(CC, MM)                                                                                                                          \
  hipLaunchKernelGGL((image_resize_kernel<CC, MM>), grid, block, 0, st, out, (long)out_img_stride, (long)out_ch_stride, out_row_stride, src, (long)src_img_stride, \
                     src_row_stride, n, H, W, oh, ow, div, add)
  if (mode == ME_RESIZE_BILINEAR) {
    me_set_kernel(C == 3 ? "image_resize_kernel<3,bilinear>" : "image_resize_kernel<1,bilinear>");
    if (C == 3) ME_RESIZE_LAUNCH(3, ME_RESIZE_BILINEAR); else ME_RESIZE_LAUNCH(1, ME_RESIZE_BILINEAR);
  } else {
    me_set_kernel(C == 3 ? "image_resize_kernel<3,nearest>" : "image_resize_kernel<1,nearest>");
    if (C == 3) ME_RESIZE_LAUNCH(3, ME_RESIZE_NEAREST); else ME_RESIZE_LAUNCH(1, ME_RESIZE_NEAREST);
  }
#undef ME_RESIZE_LAUNCH
  ME_CHECK_LAUNCH("me_image_resize")
}

// make_grid's output size: the image itself for b == 1, else cells of (h + 2) x (w + 2) in xmaps = min(n_rows, b) columns plus the 2-pixel border
static bool grid_dims(int32_t b, int32_t h, int32_t w, int32_t n_rows, int32_t* Hg, int32_t* Wg) {
  if (b == 1) {
    *Hg = h;
    *Wg = w;
    return true;
  }
  const int64_t xmaps = n_rows < b ? n_rows : b, ymaps = (b + xmaps - 1) / xmaps;
  const int64_t hg = ((int64_t)h + 2) * ymaps + 2, wg = ((int64_t)w + 2) * xmaps + 2;
  if (hg > 0x7fffffff || wg * 3 > 0x7fffffff) return false;
  *Hg = (int32_t)hg;
  *Wg = (int32_t)wg;
  return true;
}

extern "C" int me_video_grid_u8(uint8_t* out, int64_t out_frame_stride, int32_t out_row_stride, const float* vid, int64_t b_stride, int64_t c_stride,
                                int64_t f_stride, int32_t row_stride, int32_t b, int32_t c, int32_t f, int32_t h, int32_t w, int32_t n_rows, int32_t rescale,
                                void* stream) {
  if (!out || !vid) { me_set_error("me_video_grid_u8: null pointer"); return ME_EINVAL; }
  if (c != 1 && c != 3) { me_set_error("me_video_grid_u8: c must be 1 or 3"); return ME_EINVAL; }
  if (b <= 0 || f <= 0 || h <= 0 || w <= 0 || n_rows <= 0) { me_set_error("me_video_grid_u8: b, f, h, w, n_rows must be positive"); return ME_EINVAL; }
  int32_t Hg = 0, Wg = 0;
  if (!grid_dims(b, h, w, n_rows, &Hg, &Wg)) { me_set_error("me_video_grid_u8: the grid does not fit 32-bit sizes"); return ME_EINVAL; }
  if ((int64_t)Wg * 3 > out_row_stride || (int64_t)Hg * out_row_stride > out_frame_stride || w > row_stride || b_stride < 0 || c_stride < 0 || f_stride < 0 ||
      ((uintptr_t)vid & 3)) {
    me_set_error("me_video_grid_u8: strides (in elements) must hold an output row of 3 Wg bytes inside the row stride and the rows inside the frame stride; "
                 "vid 4-byte aligned with non-negative strides");
    return ME_EINVAL;
  }
  (void)hipGetLastError();
  me_set_kernel("video_grid_u8_kernel");
  const int xmaps = n_rows < b ? n_rows : b;
  hipLaunchKernelGGL(video_grid_u8_kernel, dim3(grid_for((long)f * Hg * ((Wg + PX - 1) / PX))), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out,
                     (long)out_frame_stride, out_row_stride, vid, (long)b_stride, (long)c_stride, (long)f_stride, row_stride, b, c, f, h, w, xmaps, b == 1 ? 0 : 2, Hg, Wg,
                     rescale != 0 ? 1 : 0);
  ME_CHECK_LAUNCH("me_video_grid_u8")
}
