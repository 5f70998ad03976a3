// Panorama (MultiDiffusion) around the U-Net (gfx950, fp32 latents; ABI 26): the model input of a range of overlapping views in one
// launch, and the per-pixel average of the denoised views in one launch.
//
// Reference semantics (ppdiffusers/ppdiffusers/pipelines/stable_diffusion/pipeline_stable_diffusion_panorama.py):
//   get_views                                                         :473-491
//   the slices, the circular concat, the CFG doubling, the scaling    :675-709
//   value += view, count += 1, where(count > 0, value / count, value) :736-754
//
// View geometry, shared by both kernels: ny x nx views, view v = iy * nx + ix starts at row iy * stride, column ix * stride and has
// wh x ww elements; with `circular` column j of a view is source column (ix * stride + j) mod W, rows never wrap. The C entries
// (capi.hip) hold: every window inside the source without `circular`; with it ww <= W and (nx - 1) * stride < W, so one subtraction
// of W folds a column and a view covers a source column at most once.
//
// Arithmetic. view_input is one fp32 multiply per element; view_merge is fp32 additions in ascending v onto +0.0f and one division,
// which hipcc expands to the correctly rounded sequence (v_div_scale / v_div_fmas / v_div_fixup) by default. Neither has a product
// feeding a sum, so the library's -ffp-contract=fast has nothing to contract here and the file needs no flag of its own.
#include "common.h"
#include "kernels.h"

namespace sd {
namespace {

template <int VEC>
struct Px {
  float v[VEC];
};
template <int VEC>
__device__ __forceinline__ Px<VEC> load_row(const float* p) {
  Px<VEC> r;
  if (VEC == 4) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int k = 0; k < VEC; ++k) r.v[k] = t[k];
  } else {
    r.v[0] = p[0];
  }
  return r;
}
template <int VEC>
__device__ __forceinline__ void store_row(float* p, const Px<VEC>& r) {
  if (VEC == 4) {
    f32x4 t;
#pragma unroll
    for (int k = 0; k < VEC; ++k) t[k] = r.v[k];
    *reinterpret_cast<f32x4*>(p) = t;
  } else {
    p[0] = r.v[0];
  }
}

// block (64, 4) over one window plane; grid.z = (stack sample m, channel). Sample m = (v - first) * batch + b; the plane is read once
// and written to every group, `group` floats apart. VEC == 4: W, ww and stride are multiples of 4 and both pointers 16-byte aligned,
// so a vector starts on a multiple of 4 in the source row and never straddles the wrap at W.
template <int VEC>
__global__ __launch_bounds__(256) void view_input_kernel(const float* __restrict__ x, float* __restrict__ out, float scale, int groups,
                                                         int batch, int C, int H, int W, int wh, int ww, int stride, int nx,
                                                         int first, long group) {
  const int j = (blockIdx.x * 64 + threadIdx.x) * VEC;
  const int i = blockIdx.y * 4 + threadIdx.y;
  if (j >= ww || i >= wh) return;
  const int m = blockIdx.z / C, c = blockIdx.z - m * C;
  const int v = first + m / batch, b = m % batch;
  const int iy = v / nx, ix = v - iy * nx;
  long col = (long)ix * stride + j;
  if (col >= W) col -= W;   // (circular only: without it the window lies inside the source)
  Px<VEC> p = load_row<VEC>(x + (((size_t)b * C + c) * H + ((long)iy * stride + i)) * W + col);
#pragma unroll
  for (int k = 0; k < VEC; ++k) p.v[k] *= scale;
  float* o = out + (((size_t)m * C + c) * wh + i) * ww + j;
  for (int g = 0; g < groups; ++g) store_row<VEC>(o + g * group, p);
}

// block (64, 4) over one output plane; grid.z = (image b, channel). GATHER form: an output element visits the views that cover it in
// ascending v -- rows iy0 .. iy1, in each the unwrapped columns ix0 .. ix1 and then, under `circular`, the wrapped ones ixw .. nx - 1
// (a wrapped view has ix * stride > X + W - ww >= X, so it follows every unwrapped one) -- adds their values one by one to a sum that
// starts at +0.0f, and divides by their number; no view: the sum itself. VEC == 4: W, ww and stride are multiples of 4, so four
// neighbouring columns share their covering views and are one aligned vector in each.
template <int VEC>
__global__ __launch_bounds__(256) void view_merge_kernel(const float* __restrict__ views, float* __restrict__ out, int batch, int C,
                                                         int H, int W, int wh, int ww, int stride, int ny, int nx, int circular) {
  const int X = (blockIdx.x * 64 + threadIdx.x) * VEC;
  const int Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= W || Y >= H) return;
  const int b = blockIdx.z / C, c = blockIdx.z - b * C;
  const int iy0 = Y < wh ? 0 : (Y - wh) / stride + 1, iy1 = min(ny - 1, Y / stride);
  const int ix0 = X < ww ? 0 : (X - ww) / stride + 1, ix1 = min(nx - 1, X / stride);
  const int ixw = circular ? (int)(((long)X + W - ww) / stride) + 1 : nx;
  float s[VEC];
#pragma unroll
  for (int k = 0; k < VEC; ++k) s[k] = 0.0f;
  int n = 0;
  const size_t plane = (size_t)wh * ww, sample = (size_t)C * plane;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const float* row = views + ((size_t)iy * nx * batch + b) * sample + c * plane + (size_t)(Y - iy * stride) * ww;
    for (int ix = ix0; ix <= ix1; ++ix) {
      const Px<VEC> p = load_row<VEC>(row + (size_t)ix * batch * sample + (X - ix * stride));
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] += p.v[k];
      ++n;
    }
    for (int ix = ixw; ix < nx; ++ix) {
      const Px<VEC> p = load_row<VEC>(row + (size_t)ix * batch * sample + ((long)X + W - (long)ix * stride));
#pragma unroll
      for (int k = 0; k < VEC; ++k) s[k] += p.v[k];
      ++n;
    }
  }
  Px<VEC> o;
  const float cnt = (float)n;
#pragma unroll
  for (int k = 0; k < VEC; ++k) o.v[k] = n > 0 ? s[k] / cnt : s[k];
  store_row<VEC>(out + (((size_t)b * C + c) * H + Y) * W + X, o);
}

// four elements of a row per thread where rows, windows and view origins keep 16-byte alignment
inline bool view_vec(const void* a, const void* b, int W, int ww, int stride) {
  return !(W & 3) && !(ww & 3) && !(stride & 3) && !(((uintptr_t)a | (uintptr_t)b) & 15);
}

}  // namespace

int launch_view_input(const float* x, float* out, float scale, int groups, int batch, int C, int H, int W, int wh, int ww, int stride,
                      int ny, int nx, int circular, int first, int count, hipStream_t stream) {
  // (arguments are validated by the C entry point, capi.hip)
  if (count == 0) return SD_OK;
  if ((long)count * batch * C > 65535 || (wh + 3) / 4 > 65535) return SD_ERR_UNSUPPORTED;
  const bool vec = view_vec(x, out, W, ww, stride);
  const int per = vec ? 256 : 64;
  const dim3 grid((unsigned)((ww + per - 1) / per), (unsigned)((wh + 3) / 4), (unsigned)(count * batch * C));
  const long group = (long)count * batch * C * wh * ww;
  const auto kernel = vec ? view_input_kernel<4> : view_input_kernel<1>;
  hipLaunchKernelGGL(kernel, grid, dim3(64, 4), 0, stream, x, out, scale, groups, batch, C, H, W, wh, ww, stride, nx, first, group);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

int launch_view_merge(const float* views, float* out, int batch, int C, int H, int W, int wh, int ww, int stride, int ny, int nx,
                      int circular, hipStream_t stream) {
  // (arguments are validated by the C entry point, capi.hip)
  if ((long)batch * C > 65535 || (H + 3) / 4 > 65535) return SD_ERR_UNSUPPORTED;
  const bool vec = view_vec(views, out, W, ww, stride);
  const int per = vec ? 256 : 64;
  const dim3 grid((unsigned)((W + per - 1) / per), (unsigned)((H + 3) / 4), (unsigned)(batch * C));
  const auto kernel = vec ? view_merge_kernel<4> : view_merge_kernel<1>;
  hipLaunchKernelGGL(kernel, grid, dim3(64, 4), 0, stream, views, out, batch, C, H, W, wh, ww, stride, ny, nx, circular);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd
