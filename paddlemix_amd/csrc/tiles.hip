// Tiled AutoencoderKL encode / decode (AutoencoderKL.tiled_decode / tiled_encode, PPD/models/autoencoder_kl.py:334-446): the two
// HBM-bound passes around the per-tile decoder / encoder programs.
//   tile_gather  a regular grid of equal-sized windows of an fp32 NCHW tensor -> a stack of contiguous NCHW images (the input batch
//                of one tile plan); one launch per size class of a tiling.
//   tile_blend   every element of the final tensor, written exactly once, from at most four decoded tiles.
// The reference blends sequentially and in place: tile (i, j) is blended with the finished tile above it (blend_v), then with the
// finished tile to its left (blend_h), b[p] = a[Ea - e + p] * (1 - p / e) + b[p] * (p / e) for p < e = min(Ea, Eb, ext), and is then
// cropped to [:lim, :lim]. A blend reads rows / columns of the neighbour that lie outside the neighbour's own band on that axis
// (ext <= lim), so the sequence has a closed form per output element over D = the tiles as decoded:
//   tr   = D[i-1][j](ry, x)     tl = D[i-1][j-1](ry, cx)     bl = D[i][j-1](y, cx)     cur = D[i][j](y, x)
//   top  = x in band ? lerp(tl, tr, wx) : tr                 (the tile above, after its own blend_h)
//   v    = y in band ? lerp(top, cur, wy) : cur              (blend_v)
//   left = y in band ? lerp(tl, bl, wy) : bl                 (the tile to the left, after its own blend_v)
//   out  = x in band ? lerp(left, v, wx) : v                 (blend_h)
// with lerp(a, b, w) = a * (1 - w) + b * w evaluated as the reference does: both weights formed in double and rounded to fp32, two
// fp32 products and one fp32 sum. This file is compiled with -ffp-contract=off (csrc/Makefile: the library's -ffp-contract=fast
// disregards contraction pragmas and fuses a * w0 + b * w1 into fma forms, which differ from the reference in the last bit of
// about 4 % of the blended elements), so the kernel reproduces the sequential fp32 algorithm bit for bit
// (tests/test_gpu_vae_tiling.py asserts it).
#include "common.h"
#include "kernels.h"

namespace sd {

namespace {

// position of output coordinate P (of N) on one axis of the tiling: tiles of extent min(S, N - i * lim) at stride lim
struct AxisPos {
  int i;      // tile index
  int p;      // coordinate inside tile i
  int E;      // extent of tile i
  int Ep;     // extent of tile i - 1 (i > 0)
  int e;      // blend extent against tile i - 1; 0: P is outside the band
  int q;      // coordinate inside tile i - 1 the blend reads
};

__device__ __forceinline__ AxisPos axis_pos(int P, int N, int S, int lim, int ext) {
  AxisPos a;
  a.i = P / lim;
  a.p = P - a.i * lim;
  a.E = min(S, N - a.i * lim);
  a.Ep = 0, a.e = 0, a.q = 0;
  if (a.i > 0) {
    a.Ep = min(S, N - (a.i - 1) * lim);
    const int e = min(min(a.Ep, a.E), ext);
    if (a.p < e) a.e = e, a.q = a.Ep - e + a.p;
  }
  return a;
}

// the reference's Python-float weights (1 - p / e, p / e), rounded to the tensor's fp32 when they meet it
__device__ __forceinline__ void weights(int p, int e, float& w0, float& w1) {
  const double w = (double)p / (double)e;
  w0 = (float)(1.0 - w);
  w1 = (float)w;
}

__device__ __forceinline__ float lerp_ref(float a, float b, float w0, float w1) {
  // two rounded products and a rounded sum, as the reference's tensor expression (no fma: this file's -ffp-contract=off)
  const float pa = a * w0;
  const float pb = b * w1;
  return pa + pb;
}

template <int VEC>
struct Px {
  float v[VEC];
};

template <int VEC>
__device__ __forceinline__ Px<VEC> load_px(const float* p, long sx) {
  Px<VEC> r;
  if constexpr (VEC == 4) {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(p);
      r.v[0] = t[0], r.v[1] = t[1], r.v[2] = t[2], r.v[3] = t[3];
      return r;
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) r.v[k] = p[k * sx];
  return r;
}

template <int VEC>
__device__ __forceinline__ void store_px(float* p, long sx, const Px<VEC>& r) {
  if constexpr (VEC == 4) {
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
      f32x4 t = {r.v[0], r.v[1], r.v[2], r.v[3]};
      *reinterpret_cast<f32x4*>(p) = t;
      return;
    }
  }
#pragma unroll
  for (int k = 0; k < VEC; ++k) p[k * sx] = r.v[k];
}

struct BlendArgs {
  const float* const* tiles;   // [B][ny][nx] base pointer of every decoded tile
  float* out;
  int B, C, H, W, S, lim, ext, ny, nx;
  long t_scp, t_sc, t_sx;      // tile side: element (c, y, x) of a tile of eh x ew lies at c * (t_scp * eh * ew + t_sc) + (y * ew + x) * t_sx
  long o_sb, o_sc, o_sy, o_sx; // output side: plain element strides
};

// block (64, 4): 64 threads along x (VEC elements each: one tile column, one side of the band), 4 rows; grid.z = (image, channel)
template <int VEC>
__global__ __launch_bounds__(256) void tile_blend_kernel(BlendArgs a) {
  const int X = (blockIdx.x * 64 + threadIdx.x) * VEC;
  const int Y = blockIdx.y * 4 + threadIdx.y;
  if (X >= a.W || Y >= a.H) return;
  const int b = blockIdx.z / a.C, c = blockIdx.z - b * a.C;
  const AxisPos ay = axis_pos(Y, a.H, a.S, a.lim, a.ext);
  const AxisPos ax = axis_pos(X, a.W, a.S, a.lim, a.ext);
  const float* const* row = a.tiles + ((size_t)b * a.ny + ay.i) * a.nx + ax.i;
  const long sx = a.t_sx;
  auto at = [&](const float* base, int eh, int ew, int y, int x) {
    return base + (size_t)c * (a.t_scp * eh * ew + a.t_sc) + ((size_t)y * ew + x) * sx;
  };
  Px<VEC> o = load_px<VEC>(at(row[0], ay.E, ax.E, ay.p, ax.p), sx);
  if (ay.e | ax.e) {   // inside a band: otherwise a pure copy
    float wy0 = 0.f, wy1 = 0.f;
    if (ay.e) weights(ay.p, ay.e, wy0, wy1);
    Px<VEC> tl = o, left = o;
    if (ax.e) {
      left = load_px<VEC>(at(row[-1], ay.E, ax.Ep, ay.p, ax.q), sx);
      if (ay.e) tl = load_px<VEC>(at(row[-a.nx - 1], ay.Ep, ax.Ep, ay.q, ax.q), sx);
    }
    if (ay.e) {
      const Px<VEC> tr = load_px<VEC>(at(row[-a.nx], ay.Ep, ax.E, ay.q, ax.p), sx);
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float top = tr.v[k];
        if (ax.e) {
          float wx0, wx1;
          weights(ax.p + k, ax.e, wx0, wx1);
          top = lerp_ref(tl.v[k], top, wx0, wx1);
          left.v[k] = lerp_ref(tl.v[k], left.v[k], wy0, wy1);
        }
        o.v[k] = lerp_ref(top, o.v[k], wy0, wy1);
      }
    }
    if (ax.e) {
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        float wx0, wx1;
        weights(ax.p + k, ax.e, wx0, wx1);
        o.v[k] = lerp_ref(left.v[k], o.v[k], wx0, wx1);
      }
    }
  }
  store_px<VEC>(a.out + (size_t)b * a.o_sb + (size_t)c * a.o_sc + (size_t)Y * a.o_sy + (size_t)X * a.o_sx, a.o_sx, o);
}

// block (64, 4) over one window plane; grid.z = (stack image, channel). Stack image n = first + ... is window (iy, ix) of source
// image b in the order n = (b * ny + iy) * nx + ix.
template <int VEC>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, int C, int H, int W,
                                                          int y0, int x0, int sy, int sx, int ny, int nx, int wh, int ww,
                                                          long first) {
  const int x = (blockIdx.x * 64 + threadIdx.x) * VEC;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= ww || y >= wh) return;
  const int m = blockIdx.z / C, c = blockIdx.z - m * C;
  const long n = first + m;
  const long b = n / ((long)ny * nx);
  const int t = (int)(n - b * ny * nx);
  const int iy = t / nx, ix = t - iy * nx;
  const float* s = src + (((size_t)b * C + c) * H + (y0 + iy * sy + y)) * W + (x0 + ix * sx + x);
  float* d = dst + (((size_t)m * C + c) * wh + y) * ww + x;
  store_px<VEC>(d, 1, load_px<VEC>(s, 1));
}

}  // namespace

int launch_tile_gather(const float* src, int B, int C, int H, int W, int y0, int x0, int sy, int sx, int ny, int nx, int wh, int ww,
                       long first, long count, float* dst, hipStream_t stream) {
  // (arguments are validated by the C entry point, capi.hip)
  if (count * C > 65535 || (wh + 3) / 4 > 65535) return SD_ERR_UNSUPPORTED;
  const bool vec = !(ww & 3) && !(W & 3) && !(x0 & 3) && !(sx & 3);
  const int per = vec ? 256 : 64;
  const dim3 grid((unsigned)((ww + per - 1) / per), (unsigned)((wh + 3) / 4), (unsigned)(count * C));
  if (vec)
    hipLaunchKernelGGL(tile_gather_kernel<4>, grid, dim3(64, 4), 0, stream, src, dst, C, H, W, y0, x0, sy, sx, ny, nx, wh, ww, first);
  else
    hipLaunchKernelGGL(tile_gather_kernel<1>, grid, dim3(64, 4), 0, stream, src, dst, C, H, W, y0, x0, sy, sx, ny, nx, wh, ww, first);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

int launch_tile_blend(const float* const* tiles, int B, int C, int H, int W, int S, int lim, int ext, int ny, int nx, long t_scp,
                      long t_sc, long t_sx, float* out, long o_sb, long o_sc, long o_sy, long o_sx, hipStream_t stream) {
  // (arguments are validated by the C entry point, capi.hip)
  if ((long)B * C > 65535 || (H + 3) / 4 > 65535) return SD_ERR_UNSUPPORTED;
  BlendArgs a{tiles, out, B, C, H, W, S, lim, ext, ny, nx, t_scp, t_sc, t_sx, o_sb, o_sc, o_sy, o_sx};
  // four elements of a row per thread where they share a tile and a side of the band, and rows keep 16-byte alignment
  const bool vec = t_sx == 1 && o_sx == 1 && !(W & 3) && !(S & 3) && !(lim & 3) && !(ext & 3);
  const int per = vec ? 256 : 64;
  const dim3 grid((unsigned)((W + per - 1) / per), (unsigned)((H + 3) / 4), (unsigned)(B * C));
  if (vec)
    hipLaunchKernelGGL(tile_blend_kernel<4>, grid, dim3(64, 4), 0, stream, a);
  else
    hipLaunchKernelGGL(tile_blend_kernel<1>, grid, dim3(64, 4), 0, stream, a);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd
