// The three layers of the T2I-Adapter that no other model here needs (gfx950): pixel-unshuffle fused with the NCHW fp32 -> NHWC
// element-type change its consumer needs, 2 x 2 average pooling with ceil mode, and ReLU. The adapter's convolutions are the U-Net's
// (mi355x_sd_conv3x3, mi355x_sd_linear). All three are memory-bound maps: one thread moves 8 elements, stores 16 bytes, no LDS, no
// atomics; a thread's index is 64-bit, grids are capped and strided.
//
// Reference semantics (PPD/models/adapter.py):
//   nn.PixelUnshuffle(downscale_factor)                    :306, :356, :484
//   nn.AvgPool2D(kernel_size=2, stride=2, ceil_mode=True)  :411, :537   (exclusive=True: a window over the edge averages what is inside)
//   nn.ReLU                                                :450, :571
#include "common.h"
#include "kernels.h"

namespace sd {
namespace {

constexpr long AD_MAX_BLOCKS = 8192;

inline unsigned ad_blocks(long threads) {
  const long nb = (threads + 255) / 256;
  return (unsigned)(nb > AD_MAX_BLOCKS ? AD_MAX_BLOCKS : nb);
}

// y[(b*(H/r) + i)*(W/r) + j][c*r*r + dy*r + dx] = elem(x[b][c][i*r + dy][j*r + dx]).
// R8 (r % 8 == 0, x 16-byte aligned): a thread owns 8 consecutive output columns = one run of 8 dx of one input row (32 contiguous
// bytes); consecutive threads own consecutive 16-byte groups of one output row, so a wavefront's stores are one contiguous span and
// its loads are whole dx runs (r * 4 bytes) of r / 8 ... 64 * 8 / r input rows. Otherwise: one element per thread, same order.
template <bool R8>
__global__ __launch_bounds__(256) void pixel_unshuffle_kernel(const float* __restrict__ x, int C, int H, int W, int r,
                                                              bf16* __restrict__ y, int ldy, long total) {
  const int hp = H / r, wp = W / r, rr = r * r;
  const int K = C * rr;
  const int per_row = R8 ? K >> 3 : K;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
    const long tok = id / per_row;
    const int k = (int)(id - tok * per_row) * (R8 ? 8 : 1);
    const int c = k / rr, rem = k - c * rr;
    const int dy = rem / r, dx = rem - dy * r;
    const long bi = tok / wp;                 // b * hp + i
    const int j = (int)(tok - bi * wp);
    const long b = bi / hp;
    const int i = (int)(bi - b * hp);
    const float* src = x + (((size_t)b * C + c) * H + (size_t)i * r + dy) * W + (size_t)j * r + dx;
    bf16* dst = y + (size_t)tok * ldy + k;
    if constexpr (R8) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(src), d = *reinterpret_cast<const f32x4*>(src + 4);
      const u32x4 pk = {pack_bf16(a[0], a[1]), pack_bf16(a[2], a[3]), pack_bf16(d[0], d[1]), pack_bf16(d[2], d[3])};
      *reinterpret_cast<u32x4*>(dst) = pk;
    } else {
      *dst = (bf16)*src;
    }
  }
}

__device__ __forceinline__ void ad_load8(const bf16* p, float (&o)[8]) {
  const u32x4 raw = *reinterpret_cast<const u32x4*>(p);
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(&raw);
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (float)v[j];
}

__device__ __forceinline__ void ad_store8(bf16* p, const float (&o)[8]) {
  const u32x4 pk = {pack_bf16(o[0], o[1]), pack_bf16(o[2], o[3]), pack_bf16(o[4], o[5]), pack_bf16(o[6], o[7])};
  *reinterpret_cast<u32x4*>(p) = pk;
}

// y[(b*Ho + i)*Wo + j][c] = mean of the in-bounds x[(b*H + 2i + dy)*W + 2j + dx][c], dy, dx in {0, 1}; Ho = ceil(H / 2), Wo = ceil(W / 2).
// fp32 sum in the order (0,0), (0,1), (1,0), (1,1) of those inside, times 1, 1/2 or 1/4 (exact), one rounding.
__global__ __launch_bounds__(256) void avgpool2_kernel(const bf16* __restrict__ x, int ldx, int H, int W, int cv, bf16* __restrict__ y,
                                                       int ldy, long total) {
  const int Ho = (H + 1) >> 1, Wo = (W + 1) >> 1;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
    const long pix = id / cv;
    const int c = (int)(id - pix * cv) * 8;
    const long bi = pix / Wo;                 // b * Ho + i
    const int j = (int)(pix - bi * Wo);
    const long b = bi / Ho;
    const int i = (int)(bi - b * Ho);
    const int ny = (2 * i + 1 < H) ? 2 : 1, nx = (2 * j + 1 < W) ? 2 : 1;
    const bf16* src = x + (((size_t)b * H + 2 * i) * W + 2 * j) * ldx + c;
    float acc[8], t[8];
    ad_load8(src, acc);
    if (nx == 2) {
      ad_load8(src + ldx, t);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += t[q];
    }
    if (ny == 2) {
      ad_load8(src + (size_t)W * ldx, t);
#pragma unroll
      for (int q = 0; q < 8; ++q) acc[q] += t[q];
      if (nx == 2) {
        ad_load8(src + (size_t)(W + 1) * ldx, t);
#pragma unroll
        for (int q = 0; q < 8; ++q) acc[q] += t[q];
      }
    }
    const float s = (ny * nx == 4) ? 0.25f : (ny * nx == 2) ? 0.5f : 1.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] *= s;
    ad_store8(y + (size_t)pix * ldy + c, acc);
  }
}

// y = max(x, 0) on rows of C elements; a thread reads its elements before it writes them, so y may be x. V8: 16 bytes per thread.
template <bool V8>
__global__ __launch_bounds__(256) void relu_kernel(const bf16* x, int ldx, bf16* y, int ldy, int per_row, long total) {
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
    const long row = id / per_row;
    const int c = (int)(id - row * per_row) * (V8 ? 8 : 1);
    const bf16* src = x + (size_t)row * ldx + c;
    bf16* dst = y + (size_t)row * ldy + c;
    if constexpr (V8) {
      float v[8];
      ad_load8(src, v);
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = v[q] < 0.f ? 0.f : v[q];
      ad_store8(dst, v);
    } else {
      const float v = (float)*src;
      *dst = (bf16)(v < 0.f ? 0.f : v);
    }
  }
}

int ad_fail(const char* msg) {
  set_last_error(msg);
  return SD_ERR_INVALID;
}
int ad_finish(int rc, const char* unsupported, const char* hip) {
  if (rc == SD_ERR_UNSUPPORTED) set_last_error(unsupported);
  else if (rc != SD_OK) set_last_error(hip);
  return rc;
}
inline bool ad_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int launch_pixel_unshuffle(const float* x_nchw, int B, int C, int H, int W, int r, bf16* y, int ldy, hipStream_t stream) {
  const long K = (long)C * r * r;
  if (K > 0x7fffffffL) return SD_ERR_UNSUPPORTED;
  const long toks = (long)B * (H / r) * (W / r);
  if (r % 8 == 0 && ad_aligned16(x_nchw)) {   // (W % r == 0: every run of 8 dx starts on a 32-byte boundary of x)
    const long total = toks * (K >> 3);
    hipLaunchKernelGGL(pixel_unshuffle_kernel<true>, dim3(ad_blocks(total)), dim3(256), 0, stream, x_nchw, C, H, W, r, y, ldy, total);
  } else {
    const long total = toks * K;
    hipLaunchKernelGGL(pixel_unshuffle_kernel<false>, dim3(ad_blocks(total)), dim3(256), 0, stream, x_nchw, C, H, W, r, y, ldy, total);
  }
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

int launch_avgpool2(const bf16* x, int ldx, int B, int H, int W, int C, bf16* y, int ldy, hipStream_t stream) {
  if ((C & 7) || (ldx & 7) || (ldy & 7) || !ad_aligned16(x) || !ad_aligned16(y)) return SD_ERR_UNSUPPORTED;
  const long total = (long)B * ((H + 1) / 2) * ((W + 1) / 2) * (C >> 3);
  hipLaunchKernelGGL(avgpool2_kernel, dim3(ad_blocks(total)), dim3(256), 0, stream, x, ldx, H, W, C >> 3, y, ldy, total);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

int launch_relu(const bf16* x, int ldx, bf16* y, int ldy, long rows, int C, hipStream_t stream) {
  if (!(C & 7) && !(ldx & 7) && !(ldy & 7) && ad_aligned16(x) && ad_aligned16(y)) {
    const long total = rows * (C >> 3);
    hipLaunchKernelGGL(relu_kernel<true>, dim3(ad_blocks(total)), dim3(256), 0, stream, x, ldx, y, ldy, C >> 3, total);
  } else {
    const long total = rows * C;
    hipLaunchKernelGGL(relu_kernel<false>, dim3(ad_blocks(total)), dim3(256), 0, stream, x, ldx, y, ldy, C, total);
  }
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd

extern "C" {

int mi355x_sd_pixel_unshuffle(const float* x_nchw, int B, int C, int H, int W, int r, void* y, int ldy, void* stream) {
  using namespace sd;
  if (!x_nchw || !y) return ad_fail("mi355x_sd_pixel_unshuffle: null pointer");
  if (B < 1 || C < 1 || H < 1 || W < 1 || r < 1) return ad_fail("mi355x_sd_pixel_unshuffle: needs B, C, H, W, r >= 1");
  if (H % r || W % r) return ad_fail("mi355x_sd_pixel_unshuffle: H and W must be multiples of r");
  if ((int64_t)ldy < (int64_t)C * r * r) return ad_fail("mi355x_sd_pixel_unshuffle: ldy must be at least C * r * r");
  if ((ldy & 7) || !ad_aligned16(y)) return ad_fail("mi355x_sd_pixel_unshuffle: ldy must be a multiple of 8 and y 16-byte aligned");
  return ad_finish(launch_pixel_unshuffle(x_nchw, B, C, H, W, r, (bf16*)y, ldy, reinterpret_cast<hipStream_t>(stream)),
                   "mi355x_sd_pixel_unshuffle: unsupported shape (C * r * r < 2^31)", "mi355x_sd_pixel_unshuffle: HIP launch failed");
}

int mi355x_sd_avgpool2(const void* x, int ldx, int B, int H, int W, int C, void* y, int ldy, void* stream) {
  using namespace sd;
  if (!x || !y) return ad_fail("mi355x_sd_avgpool2: null pointer");
  if (B < 1 || H < 1 || W < 1 || C < 1) return ad_fail("mi355x_sd_avgpool2: needs B, H, W, C >= 1");
  if (ldx < C || ldy < C) return ad_fail("mi355x_sd_avgpool2: ldx and ldy must be at least C");
  return ad_finish(launch_avgpool2((const bf16*)x, ldx, B, H, W, C, (bf16*)y, ldy, reinterpret_cast<hipStream_t>(stream)),
                   "mi355x_sd_avgpool2: C, ldx, ldy must be multiples of 8 and x, y 16-byte aligned", "mi355x_sd_avgpool2: HIP launch failed");
}

int mi355x_sd_relu(const void* x, int ldx, void* y, int ldy, int64_t rows, int C, void* stream) {
  using namespace sd;
  if (!x || !y) return ad_fail("mi355x_sd_relu: null pointer");
  if (rows < 1 || C < 1) return ad_fail("mi355x_sd_relu: needs rows >= 1 and C >= 1");
  if (ldx < C || ldy < C) return ad_fail("mi355x_sd_relu: ldx and ldy must be at least C");
  return ad_finish(launch_relu((const bf16*)x, ldx, (bf16*)y, ldy, (long)rows, C, reinterpret_cast<hipStream_t>(stream)), "mi355x_sd_relu: unsupported",
                   "mi355x_sd_relu: HIP launch failed");
}

}  // extern "C"
