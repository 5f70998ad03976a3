// The reference's fused custom ops of the SD3 / DiT path with THEIR signatures (seam B4), as stand-alone HBM-bound kernels:
//   fused_adaLN_scale_residual(x, mha_out, gate_msa, scale_mlp, shift_mlp, weight, bias, epsilon) -> (resi_out, adaLN_out)
//       paddlemix/triton_ops/triton_ops.py:758-920; unfused definition :842-847:
//       resi_out = mha_out * gate[:, None] + x ;  adaLN_out = layer_norm(resi_out, weight, bias, eps) * (1 + scale[:, None]) + shift[:, None]
//   split_concat(x [B,S1,3C], y [B,S2,3C]) -> (q, k, v), each [B, S1+S2, C] = concat(x chunk i, y chunk i) along the sequence
//       triton_ops.py:1692-1752 (kernel :1652-1689)
// Inside this library's own SD3 program the same arithmetic lives in GEMM epilogues / row maps (sd3.py); these entry points exist
// so that a PaddleMIX maintainer can swap the Triton ops one for one.
// One wave per row, 16-byte accesses, fp32 statistics (the shifted one-pass row_moments of norm_rows.h), two outputs written in the
// pass that read the inputs: 2 reads + 2 writes of the row = the op's minimum traffic.
#include "common.h"
#include "kernels.h"
#include "norm_rows.h"

namespace sd {

// Not a form of row_norm_kernel (written as one, every instantiation compiled to more registers: profiles/r16_row_norm_skeleton.txt):
// the body below stands on the skeleton's pieces -- RowWave, row_moments at one row per trip, pack8 / store8, the launcher.
// M16: gate / scale / shift / weight / bias are the build's 16-bit element type (what the reference passes) instead of fp32
template <bool M16>
struct FusedAdaLN {
  const bf16* x;
  int ldx;
  const bf16* mha;
  int ldm;
  const void *gate, *scale, *shift;
  int ld_mod, rows_per_batch;
  const void *weight, *bias;   // either may be null
  bf16* resi;
  int ldr;
  bf16* out;
  int ldo;
};

template <bool M16, int NCH>
__global__ __launch_bounds__(256) void fused_adaln_scale_residual_kernel(FusedAdaLN<M16> f, int rows, int C, float eps) {
  const RowWave w(C);
  const int wave_g = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * (blockDim.x >> 6);
  for (int row = wave_g; row < rows; row += nwaves) {
    const size_t mrow = (size_t)(row / f.rows_per_batch) * f.ld_mod;
    float v[1][NCH][8];
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cc = w.lane + 64 * i;
      if (cc < w.cv) {
        const u32x4 rx = *reinterpret_cast<const u32x4*>(f.x + (size_t)row * f.ldx + cc * 8);
        const u32x4 rm = *reinterpret_cast<const u32x4*>(f.mha + (size_t)row * f.ldm + cc * 8);
        const bf16x8 tx = *reinterpret_cast<const bf16x8*>(&rx), tm = *reinterpret_cast<const bf16x8*>(&rm);
        float g8[8], r8[8];
        load_mod8<M16>(f.gate, mrow + cc * 8, g8);
#pragma unroll
        for (int j = 0; j < 8; ++j) r8[j] = __builtin_fmaf((float)tm[j], g8[j], (float)tx[j]);
        // the residual leaves as a 16-bit tensor; the LayerNorm of the unfused definition sees THAT tensor
        const u32x4 pk = pack8(r8);
        *reinterpret_cast<u32x4*>(f.resi + (size_t)row * f.ldr + cc * 8) = pk;
#pragma unroll
        for (int j = 0; j < 8; ++j) v[0][i][j] = chunk_val(pk, j);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[0][i][j] = 0.f;
      }
    }
    float mean[1], rstd[1];
    row_moments(v, w, eps, mean, rstd);
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int cc = w.lane + 64 * i;
      if (cc < w.cv) {
        float sc[8], sh[8], wv[8], bv[8], o[8];
        load_mod8<M16>(f.scale, mrow + cc * 8, sc);
        load_mod8<M16>(f.shift, mrow + cc * 8, sh);
        if (f.weight) load_mod8<M16>(f.weight, (size_t)cc * 8, wv);
        if (f.bias) load_mod8<M16>(f.bias, (size_t)cc * 8, bv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float y = (v[0][i][j] - mean[0]) * rstd[0];
          if (f.weight) y *= wv[j];
          if (f.bias) y += bv[j];
          o[j] = __builtin_fmaf(y, 1.0f + sc[j], sh[j]);
        }
        store8(f.out + (size_t)row * f.ldo + cc * 8, o);
      }
    }
  }
}
template <bool M16, int NCH>
struct RowKernel<FusedAdaLN<M16>, NCH, 1> {
  static constexpr auto fn = fused_adaln_scale_residual_kernel<M16, NCH>;
};

int launch_fused_adaln_scale_residual(const bf16* x, int ldx, const bf16* mha, int ldm, const void* gate, const void* scale,
                                      const void* shift, int ld_mod, int mod16, int rows_per_batch, const void* weight,
                                      const void* bias, float eps, int rows, int C, bf16* resi, int ldr, bf16* out, int ldo,
                                      hipStream_t stream) {
  if (rows <= 0 || C <= 0 || rows_per_batch <= 0) return SD_ERR_INVALID;
  if ((C & 7) || (ldx & 7) || (ldm & 7) || (ldr & 7) || (ldo & 7) || (ld_mod & (mod16 ? 7 : 3)) || C > 4096) return SD_ERR_UNSUPPORTED;
  if (mod16 && ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(bias)) & 15)) return SD_ERR_UNSUPPORTED;
  const int blocks = one_row_grid(rows);
  if (mod16)
    return launch_row_norm<Inst<2, 1>, Inst<4, 1>, Inst<8, 1>>(
        FusedAdaLN<true>{x, ldx, mha, ldm, gate, scale, shift, ld_mod, rows_per_batch, weight, bias, resi, ldr, out, ldo}, rows, C, eps,
        blocks, "fused_adaln", "m16", stream);
  return launch_row_norm<Inst<2, 1>, Inst<4, 1>, Inst<8, 1>>(
      FusedAdaLN<false>{x, ldx, mha, ldm, gate, scale, shift, ld_mod, rows_per_batch, weight, bias, resi, ldr, out, ldo}, rows, C, eps,
      blocks, "fused_adaln", "m32", stream);
}


// out_i[b][s][:] = (s < S1 ? x[b][s] : y[b][s - S1])[i*C : (i+1)*C], i = 0 (q), 1 (k), 2 (v)
__global__ void split_concat_kernel(const bf16* __restrict__ x, const bf16* __restrict__ y, bf16* __restrict__ o0,
                                    bf16* __restrict__ o1, bf16* __restrict__ o2, int B, int S1, int S2, int cv) {
  const long total = (long)B * (S1 + S2) * 3 * cv;
  for (long id = (long)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (long)gridDim.x * blockDim.x) {
    const int cc = (int)(id % cv);
    const long t = id / cv;
    const int i = (int)(t % 3);
    const long rs = t / 3;                    // b * (S1 + S2) + s
    const int s = (int)(rs % (S1 + S2));
    const long b = rs / (S1 + S2);
    const bf16* src = (s < S1) ? x + ((b * S1 + s) * 3 + i) * (size_t)cv * 8 : y + ((b * S2 + (s - S1)) * 3 + i) * (size_t)cv * 8;
    bf16* dst = (i == 0 ? o0 : i == 1 ? o1 : o2) + (size_t)rs * cv * 8;
    *reinterpret_cast<u32x4*>(dst + cc * 8) = *reinterpret_cast<const u32x4*>(src + cc * 8);
  }
}

int launch_split_concat(const bf16* x, const bf16* y, bf16* o0, bf16* o1, bf16* o2, int B, int S1, int S2, int C, hipStream_t stream) {
  if (B <= 0 || S1 < 0 || S2 < 0 || S1 + S2 <= 0 || C <= 0) return SD_ERR_INVALID;
  if (C & 7) return SD_ERR_UNSUPPORTED;
  const long total = (long)B * (S1 + S2) * 3 * (C >> 3);
  long nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(split_concat_kernel, dim3((unsigned)nb), dim3(256), 0, stream, x, y, o0, o1, o2, B, S1, S2, C >> 3);
  return hipGetLastError() == hipSuccess ? SD_OK : SD_ERR_HIP;
}

}  // namespace sd
