/* mi355x_sd.h — C ABI of libmi355x_sd.so: the MI355X (gfx950) implementation of the ppdiffusers
 * Stable-Diffusion denoising hot path (UNet2DConditionModel forward).
 *
 * This is the drop-in boundary.  Every entry point is `extern "C"`, takes plain device pointers, sizes and a
 * hipStream_t (passed as void*), allocates nothing, is stream-ordered and is safe to capture in a hipGraph.
 * All functions return 0 on success or a non-zero MI355X_SD_ERR_* code; mi355x_sd_last_error() gives the text.
 *
 * The reference (PaddlePaddle/PaddleMIX @ 2024-10-24) reaches this arithmetic through Paddle ops and its own
 * custom-op mechanism; each entry point cites the reference interface it replaces (paths relative to the
 * reference checkout; PPD/ = ppdiffusers/ppdiffusers/):
 *   - the custom-op ABI itself: PD_BUILD_OP(...).SetKernelFn(...) + paddle::Tensor arguments,
 *     paddlemix/triton_ops/triton_ops.py:641-693, 926-972; Paddle is not available for AMD here, so the tensor
 *     arguments become (pointer, shape, stride) triples.  INTEGRATION.md shows the PD_BUILD_OP / ctypes stub a
 *     maintainer would add on the reference side.
 *
 * Conventions
 *   - activations: bf16, token-major rows [rows][C] == NHWC, with an explicit row stride `ld*` in elements
 *     (a channel concat is two producers writing one buffer); C and all strides multiples of 8.
 *   - weights: bf16 [N][K] with K contiguous (a Paddle Linear weight [in,out] transposed once at load;
 *     a conv weight OIHW repacked to [O][kh][kw][I]); biases / norm affine parameters: fp32.
 *   - accumulation and all statistics in fp32.
 */
#ifndef MI355X_SD_H
#define MI355X_SD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MI355X_SD_ABI_VERSION 26
#define MI355X_SD_OK 0
#define MI355X_SD_ERR_INVALID 1      /* bad argument (shape <= 0, null pointer ...)          */
#define MI355X_SD_ERR_UNSUPPORTED 2  /* well-formed but outside the implemented configurations */
#define MI355X_SD_ERR_HIP 3          /* HIP runtime error; see mi355x_sd_last_error()          */

int mi355x_sd_abi_version(void);
/* 16-bit element type of this build: the library comes in two builds of the same sources, libmi355x_sd.so (bfloat16,
 * the dtype of BASELINE.json's configurations) and libmi355x_sd_f16.so (IEEE half: same speed, 3 more mantissa bits,
 * the dtype the reference's own GPU pipelines default to -- paddle_dtype=paddle.float16). Wherever this header says
 * "bf16" read "the element type of the build". */
#define MI355X_SD_ELEM_BF16 0
#define MI355X_SD_ELEM_F16 1
int mi355x_sd_elem_dtype(void);
const char* mi355x_sd_last_error(void);
/* Selects `device` and verifies it is a gfx950 part. */
int mi355x_sd_init(int device);

/* SCRATCH OF THE GEMM-CLASS CALLS (ABI 12): mi355x_sd_linear, _linear_ex, _linear_ln and mi355x_sd_conv3x3 take `ws, ws_bytes` --
 * caller-owned device memory, 16-byte aligned, or NULL / 0 -- as ARGUMENTS (until ABI 11 a process-wide binding,
 * mi355x_sd_set_workspace, whose stale pointer a later call could write through; it is gone). The scratch belongs to the call:
 * launches that run concurrently (two streams, two handles) must be given different buffers, launches ordered on one stream may
 * share one. The model handles own theirs (mi355x_sd_unet_*: part of the arena bound with _bind_workspace; mi355x_sd_program_*: a
 * scratch region of the program). Two uses:
 *   split-K: launches that cannot fill the 256 CUs (batch-1 SD-1.5: 64..1024 rows against K up to 23040) split K over blockIdx.y,
 *     store fp32 slices here and reduce them in fixed order (deterministic); the split count is bounded by ws_bytes, so the same
 *     call with another ws_bytes may sum in another order (results equal to fp32 rounding, bit-stable for a fixed size);
 *   weight-only fp8 (mi355x_sd_linear_ex, w_scale != NULL): launches of M >= 4096 rows and more than 128 tiles widen the e4m3
 *     matrix once, just in time, into the first 2 * N * K bytes (up to ~19 MB for SD3-medium's 6144 x 1536 matrices) and multiply
 *     with the 16-bit kernels; a smaller scratch is not an error -- the launch takes the slower path that converts in the fragment
 *     load (same result to fp32 rounding).
 * NULL: neither path. 32 MiB covers every model of this repository. The library never allocates ("no hidden allocation"). A
 * pointer the HIP runtime does not know as device (or managed) memory is refused with MI355X_SD_ERR_INVALID before anything is
 * launched: the kernels write through it. */

/* ---- seam B1: the whole UNet2DConditionModel behind one handle (paddlemix_amd/csrc/unet_exec.hip) ----------------------------
 * What a compiled host (Paddle C++, a serving runtime) binds instead of the per-op entry points: the reference calls its UNet once
 * per denoising step as `unet(sample, t, encoder_hidden_states, added_cond_kwargs=...)` (pipeline_stable_diffusion.py:866-879) and
 * its deployment pipelines already treat it as an opaque predictor with named inputs (PaddleInferRuntimeModel.__call__,
 * PPD/models/paddleinfer_runtime.py:47-126; input names PPD/../deploy/sd15/export_model.py:78-90). Life cycle:
 *   create(config.json text) -> load_weight(name, host pointer) for every parameter (reference names, Paddle layouts: Linear
 *   [in,out], conv OIHW; enumerate them with num_params / param_info) -> weight_bytes -> finalize_weights(caller's device buffer)
 *   -> plan(B, H, W, L) -> bind_workspace(caller's device buffer) -> forward(...) per step -> destroy.
 * The library never allocates device memory; all tensors of forward() are device pointers; split-K GEMMs use the workspace of
 * mi355x_sd_set_workspace like the per-op calls. Built: the four SD block types, conv / linear projections, addition_embed_type
 * None | "text_time"; anything else in the config is refused at create (MI355X_SD_ERR_UNSUPPORTED), never ignored. */
#define MI355X_SD_DTYPE_F32 0
#define MI355X_SD_DTYPE_BF16 1
#define MI355X_SD_DTYPE_F16 2
int mi355x_sd_unet_create(const char* config_json, void** handle);
int mi355x_sd_unet_destroy(void* handle);
/* options: "residual_f32" = 1 (before plan) keeps the residual stream in fp32 (MI355X_SD_R_F32); "fold_softmax_scale" = 0 | 1 (default 1;
 * before the weights are packed): head_dim^-0.5 * log2(e) is folded into the self-attention to_q weights (head_dim 64) and those attentions
 * run as MI355X_SD_SDPA_LOG2 */
int mi355x_sd_unet_set_option(void* handle, const char* key, int value);
int mi355x_sd_unet_num_params(void* handle);
int mi355x_sd_unet_param_info(void* handle, int index, const char** name, int64_t* shape4, int* ndim);
int mi355x_sd_unet_load_weight(void* handle, const char* name, const void* host_ptr, const int64_t* shape, int ndim, int dtype);
int mi355x_sd_unet_weight_bytes(void* handle, size_t* bytes);
int mi355x_sd_unet_finalize_weights(void* handle, void* device_buffer, size_t bytes, void* stream);
/* finalize_weights in two halves for hosts that stage uploads themselves: the packed image into HOST memory, then the device
 * address it was copied to. packed_tensor locates one packed tensor inside the image (keys as in paddlemix_amd/unet.py). */
int mi355x_sd_unet_pack_weights(void* handle, void* host_buffer, size_t bytes);
int mi355x_sd_unet_attach_weights(void* handle, void* device_buffer, size_t bytes);
int mi355x_sd_unet_packed_tensor(void* handle, const char* key, size_t* offset, size_t* bytes, int* rows, int* cols);
int mi355x_sd_unet_plan(void* handle, int B, int H, int W, int L, size_t* workspace_bytes);
int mi355x_sd_unet_bind_workspace(void* handle, void* device_ptr, size_t bytes);
int mi355x_sd_unet_num_launches(void* handle);
/* All pointers are device memory, fp32: sample [B,Cin,H,W], timestep [1], encoder_hidden_states [B,L,D], text_embeds
 * [B, projection_class_embeddings_input_dim - 6*addition_time_embed_dim] and time_ids [B,6] (text_time only, else NULL), in_scale
 * optional scalar multiplied into the sample (scheduler.scale_model_input; NULL = 1), out [B,Cout,H,W]. Missing text_embeds /
 * time_ids on a text_time model is MI355X_SD_ERR_INVALID (the reference's ValueError, unet_2d_condition.py:993-1001).
 * use_graph != 0: the launches are captured into a hipGraph on the first call and replayed afterwards. */
int mi355x_sd_unet_forward(void* handle, void* stream, const float* sample, const float* timestep,
                           const float* encoder_hidden_states, const float* text_embeds, const float* time_ids,
                           const float* in_scale, float* out, int use_graph);
/* The optional inputs of UNet2DConditionModel.forward that change the PROGRAM are chosen at plan time (plan_ex flags), their
 * tensors are handed over per call (forward_ex; a NULL / absent input whose flag was planned is MI355X_SD_ERR_INVALID, as is a
 * non-NULL one that was not planned):
 *   ENC_MASK   encoder_attention_mask [B, L], 1 = attend, 0 = masked: becomes the additive bias (1 - m) * -10000 of every
 *              cross-attention (unet_2d_condition.py:925-927)
 *   SELF_MASK  attention_mask [B, H*W]: the same for every self-attention (:916-923). Like the reference, this only works for a
 *              UNet whose attention levels all see H*W tokens; a level with another token count fails the plan (the reference
 *              fails on the shapes of the add)
 *   CONTROLNET down_block_additional_residuals (one fp32 NCHW tensor per skip connection, in the order the down path produces
 *              them: conv_in first) + mid_block_additional_residual (:1121-1132, 1151-1155), e.g. the outputs of
 *              ControlNetModel; both or neither. Down residuals without the mid one are the reference's deprecated T2I-Adapter form
 *              (:1084-1094): MI355X_SD_ERR_UNSUPPORTED here -- the intrablock adds (down_intrablock_additional_residuals, ABI 23)
 *              are planned by the Python planner only
 * class_labels, timestep_cond and the IP-Adapter image_embeds: mi355x_sd_unet_set_input below. */
#define MI355X_SD_UNET_ENC_MASK 1
#define MI355X_SD_UNET_SELF_MASK 2
#define MI355X_SD_UNET_CONTROLNET 4
int mi355x_sd_unet_plan_ex(void* handle, int B, int H, int W, int L, int flags, size_t* workspace_bytes);
/* number of skip tensors = length of down_block_additional_residuals, and the [C, H, W] of skip i (i == count: the mid output) */
int mi355x_sd_unet_num_skips(void* handle);
int mi355x_sd_unet_skip_shape(void* handle, int index, int* C, int* H, int* W);
int mi355x_sd_unet_forward_ex(void* handle, void* stream, const float* sample, const float* timestep,
                              const float* encoder_hidden_states, const float* text_embeds, const float* time_ids,
                              const float* in_scale, const float* encoder_attention_mask, const float* attention_mask,
                              const float* const* down_block_additional_residuals, int num_down_residuals,
                              const float* mid_block_additional_residual, float* out, int use_graph);
/* The tensor inputs of UNet2DConditionModel.forward that belong to the CONFIG -- a model built with a class embedding or with
 * time_cond_proj_dim reads them in every forward (unet_2d_condition.py:953-975; embeddings.py:284-285) -- are bound by name, not
 * passed per call: device pointers, read (copied into the plan's static buffers, on the call's stream) by every forward[_ex] call
 * from then on, until replaced; NULL unbinds.
 *   "class_labels"   class_embed_type null + num_class_embeds: int32 [B], the row of the nn.Embedding table per sample -- every
 *                    label must lie in [0, num_class_embeds): the gather reads the table at the index it is given, unchecked;
 *                    "timestep": fp32 [B] (goes through time_proj and a TimestepEmbedding); "projection" / "simple_projection":
 *                    fp32 [B, projection_class_embeddings_input_dim]; "identity": fp32 [B, 4 * block_out_channels[0]].
 *                    A forward call of such a model with nothing bound is MI355X_SD_ERR_INVALID (the reference's ValueError,
 *                    :954-955). class_embeddings_concat=true hands the blocks [emb | class_emb] (:443-449, 972-975); together with
 *                    addition_embed_type it is refused at create, as by the Python planner.
 *   "timestep_cond"  fp32 [B, time_cond_proj_dim] (the LCM guidance-scale embedding); unbound = the reference's None (no term).
 *   "image_embeds"   fp32 [B, encoder_hid_dim] of a model with encoder_hid_dim_type "ip_image_proj" (the CLIP image embedding of the
 *                    IP-Adapter prompt, added_cond_kwargs["image_embeds"], :1054-1061): projected to ip_adapter_num_tokens image
 *                    tokens (ImageProjection, embeddings.py:507-518) whose attention is added to every cross-attention output with
 *                    the IP-Adapter scale (IPAdapterAttnProcessor, attention_processor.py:1816-1900). Unbound at a forward call =
 *                    MI355X_SD_ERR_INVALID (the reference's ValueError).
 * Binding an input the model does not have is MI355X_SD_ERR_INVALID. */
int mi355x_sd_unet_set_input(void* handle, const char* name, const void* device_ptr);
/* IPAdapterAttnProcessor.scale of every cross-attention (the reference's set_ip_adapter_scale, loaders/ip_adapter.py; default 1; 0
 * drops the image-token attention launches). A constant of the planned launches: changing it discards the plan -- plan and bind again. */
int mi355x_sd_unet_set_ip_adapter_scale(void* handle, float scale);
/* FreeU (the reference's UNet2DConditionModel.enable_freeu / disable_freeu, unet_2d_condition.py:777-808; ABI 22): enabled != 0 plans
 * one mi355x_sd_freeu launch in front of every resnet of up blocks 0 (b1, s1) and 1 (b2, s2); enabled == 0 plans none (the default).
 * The four values must be finite. Constants of the planned launches: a change discards the plan -- plan and bind again. */
int mi355x_sd_unet_set_freeu(void* handle, int enabled, float s1, float s2, float b1, float b2);
/* ---- seam B2: any exported step program behind one handle (paddlemix_amd/csrc/program_exec.hip) --------------------------------
 * Every model of the path (UNet2DConditionModel, ControlNetModel, SD3Transformer2DModel, the DiT Transformer2DModel, AutoencoderKL
 * decode / encode, the CLIP and T5 text encoders) runs as a static list of the per-op launches below over weights + scratch. The
 * Python planners build that list; `paddlemix_amd.export.export_program(model, plan, path)` writes it to a file (entry-point
 * names, arguments with every device pointer as (region, offset), packed weights, plan-time constants, the named input / output
 * regions), and a host without Python replays it -- the shape of the reference's own deployment path: export offline
 * (PPD/../deploy/sd15/export_model.py:78-90), then run behind a predictor with named inputs
 * (PaddleInferRuntimeModel.__call__, PPD/models/paddleinfer_runtime.py:47-126: get_input_handle / copy_from_cpu / run / copy_to_cpu):
 *   load(path)  host only: parses and type-checks every launch against this library's entry points (refuses another ABI version
 *               or the other 16-bit element build) -> device_bytes -> bind(caller's device buffer, 256-byte aligned: uploads
 *               weights and constants, resolves the pointers) -> io_info(i): name, direction, dtype, shape and DEVICE ADDRESS of
 *               each input / output region (copy inputs there, in the dtype it names) -> run(stream) per call -> destroy.
 * The library allocates no device memory; run() binds the split-K workspace the program was planned with (inside the same
 * buffer), so it reproduces the exporting process bit for bit. Option "use_graph" = 1: the replay becomes one hipGraph. */
#define MI355X_SD_IO_F32 0
#define MI355X_SD_IO_ELEM16 1   /* the build's 16-bit element type (mi355x_sd_elem_dtype) */
#define MI355X_SD_IO_I32 2
#define MI355X_SD_IO_U8 3
int mi355x_sd_program_load(const char* path, void** handle);
int mi355x_sd_program_destroy(void* handle);
int mi355x_sd_program_set_option(void* handle, const char* key, int value);
int mi355x_sd_program_num_launches(void* handle);
int mi355x_sd_program_device_bytes(void* handle, size_t* bytes);
int mi355x_sd_program_bind(void* handle, void* device_buffer, size_t bytes, void* stream);
int mi355x_sd_program_num_io(void* handle);
int mi355x_sd_program_io_info(void* handle, int index, const char** name, int* is_output, int* dtype, int64_t* shape4, int* ndim,
                              size_t* bytes, void** device_ptr);
int mi355x_sd_program_run(void* handle, void* stream);

/* bias[i] = (1 - mask[i]) * -10000: the additive form of a keep-mask (unet_2d_condition.py:921-927) */
int mi355x_sd_mask_to_bias(const float* mask, float* bias, int64_t n, void* stream);

/* flags for mi355x_sd_linear / mi355x_sd_conv3x3 */
#define MI355X_SD_GEGLU 1    /* W/bias rows interleaved [16 value | 16 gate]; writes N/2 columns value*gelu_erf(gate) */
#define MI355X_SD_OUT_F32 2  /* C is fp32 */
#define MI355X_SD_GELU_TANH 8 /* tanh-GELU applied to the final value (FeedForward "gelu-approximate", PPD/models/attention.py:648-649) */
#define MI355X_SD_SILU 4     /* SiLU applied to the final value (TimestepEmbedding.act, PPD/models/embeddings.py:283-295) */
#define MI355X_SD_R_F32 32   /* R is fp32 rows (ldr in fp32 elements): the fp32 residual-stream mode, where the tensors the reference
                              * adds onto (`hidden_states + input_tensor` resnet.py:806, `attn_output + hidden_states` attention.py:430,
                              * 455, 487, transformer_2d.py:467) never round to 16 bits; combine with MI355X_SD_OUT_F32 */
#define MI355X_SD_CONV_KB64 64 /* conv3x3, Cin % 64 == 0: W is packed [O][Cin/64][3][3][64] instead of [O][3][3][Cin] -- the K loop then walks the 9
                              * taps of one 64-channel block back to back, so the eight re-reads of a [pixels x 64 channels] region hit the XCD's
                              * L2 (32 KB per block) instead of coming back through the fabric a full channel sweep later (measured: profiles/HISTORY.md section 5) */
#define MI355X_SD_PAD_BR 16  /* conv3x3, stride 2 only: zero padding is one row / column at the bottom / right instead of all round
                              * (Downsample2D with padding=0: F.pad (0,1,0,1) then an unpadded conv, PPD/models/resnet.py:277-279 --
                              * the VAE encoder's downsamplers, vae.py:113) */

/* C[M,N] = ((A[M,K] . W[N,K]^T) + bias[N] + rowbias[m / rows_per_batch][N] + R[M,N]) * out_scale
 * Replaces LoRACompatibleLinear.forward (PPD/models/lora.py:453-459) and, with conv1x1 weights, the 1x1
 * LoRACompatibleConv (lora.py:364-377); GEGLU = PPD/models/activations.py:101-104 fused into the epilogue;
 * R / out_scale = the residual adds of PPD/models/attention.py:429,459,485 and resnet.py:800-806.
 * bias, rowbias, R may be NULL. */
int mi355x_sd_linear(const void* A, int lda, const void* W, void* C, int ldc, int M, int N, int K,
                     const float* bias, const float* rowbias, int rows_per_batch, int ld_rowbias,
                     const void* R, int ldr, float out_scale, int flags, void* ws, size_t ws_bytes, void* stream);

/* mi355x_sd_linear plus what the SD3 MMDiT blocks (PPD/models/attention.py:164-214, attention_processor.py:916-983) need:
 *   gate  : out = R + gate[m / rows_per_batch][n] * (acc + bias)     (adaLN-Zero gated residuals, attention.py:181-196)
 *   a_/c_ rows_per_batch + batch_stride: row m of A (C) lives at (m / rpb) * batch_stride + (m % rpb) * lda (ldc) -- the
 *   w_scale != NULL: W is OCP fp8 e4m3 [N][K] (one byte per element) with a per-output-channel fp32 scale, W ~ w_scale[n] * q;
 *     every w_scale[n] must be > 0 (clamp an all-zero channel's absmax / 448 to a tiny positive number, as the library's own
 *     quantiser does): the widened path starts the accumulators at bias[n] / w_scale[n];
 *   the kernel widens q to bf16 in registers (exact) and scales the fp32 accumulator (weight-only fp8: BASELINE config 5).
 *   projections of the image and the text tokens read / write one joint [B, S_img + S_txt, .] buffer in place, which is
 *   the fused split + concat of paddlemix/triton_ops/triton_ops.py:1652-1752 (split_concat) folded into the GEMMs. */
int mi355x_sd_linear_ex(const void* A, int lda, int a_rows_per_batch, int64_t a_batch_stride, const void* W,
                        const float* w_scale, void* C,
                        int ldc, int c_rows_per_batch, int64_t c_batch_stride, int M, int N, int K, const float* bias,
                        const float* rowbias, int ld_rowbias, const float* gate, int ld_gate, int rows_per_batch,
                        const void* R, int ldr, float out_scale, int flags, void* ws, size_t ws_bytes, void* stream);

/* LayerNorm folded into the consuming projection (BasicTransformerBlock: norm1 -> attn1.to_q/k/v, norm2 -> attn2.to_q,
 * norm3 -> ff.net.0.proj; PPD/models/attention.py:405-486).  With W' = W diag(gamma) (bf16), w_rowsum[n] = sum_k W'[n][k]
 * and bias' = bias + W beta prepared at load time,
 *     LN(x) W^T + bias  =  rstd[m] * (x W'^T)[m][n] - mean[m] * rstd[m] * w_rowsum[n] + bias'[n],
 * so the normalised activation is never written to or re-read from HBM: mi355x_sd_row_stats reads the rows once and
 * stores row_stats[m] = (rstd, -mean * rstd) (fp32 pairs), mi355x_sd_linear_ln multiplies the RAW rows and applies the
 * correction to its fp32 accumulators before bias / GEGLU / activation flags. */
int mi355x_sd_row_stats(const void* x, int rows, int C, int ldx, float eps, float* row_stats, void* stream);
int mi355x_sd_linear_ln(const void* A, int lda, const float* row_stats, const void* W, const float* w_rowsum, void* C,
                        int ldc, int M, int N, int K, const float* bias, int flags, void* ws, size_t ws_bytes, void* stream);

/* ---- W8A8: fp8 (OCP e4m3) MFMA path of the MMDiT block GEMMs (BASELINE config 5: "fp8 weights ... CDNA4 fp8 MFMA") ----
 * C[M,N] = (A8 . W8^T) * a_scale[m] * w_scale[n] + bias, then optional gate[m / rows_per_batch][n] * (.) + R, optional
 * tanh-GELU; bf16 output. A8 [M,K] / W8 [N,K] are e4m3 bytes, K % 128 == 0 (one v_mfma_scale_f32_16x16x128_f8f6f4 per
 * 16x16 tile and K-tile), lda in elements (= bytes), % 16; a_rows_per_batch / c_rows_per_batch as in mi355x_sd_linear_ex.
 * Scales: value = scale * q with scale = absmax / 448 per A row (mi355x_sd_adaln_f8 / mi355x_sd_quantize_rows) and per
 * output channel of W (quantised at load). The reference has no fp8 inference path; parity is defined against the oracle
 * evaluated on the same quantised operands (tests/test_gpu_sd3.py) and the quantisation error itself is reported. */
int mi355x_sd_linear_f8(const void* A8, int lda, int a_rows_per_batch, int64_t a_batch_stride, const float* a_scale,
                        const void* W8, const float* w_scale, void* C, int ldc, int c_rows_per_batch,
                        int64_t c_batch_stride, int M, int N, int K, const float* bias, const float* gate, int ld_gate,
                        int rows_per_batch, const void* R, int ldr, int flags, void* stream);
/* mi355x_sd_adaln with the e4m3 quantisation fused: y8[row][C] bytes (row stride ldy bytes), y_scale[row]; y_l2
 * (optional) receives the row's L2 norm before quantisation (see mi355x_sd_linear_f8_q). */
int mi355x_sd_adaln_f8(const void* x, int rows, int C, int ldx, const float* scale, const float* shift, int ld_mod,
                       int rows_per_batch, float eps, void* y8, int ldy, float* y_scale, float* y_l2, void* stream);
/* W8A8 GEMM with an e4m3 OUTPUT for the next GEMM (ff.net.0 -> tanh-GELU -> ff.net.2 without a re-quantisation pass):
 * C8[m][n] = e4m3(act(acc * a_scale[m] * w_scale[n] + bias[n]) / c_scale[m]). The output row scale needs no pass over
 * the row: |acc + bias| <= a_l2[m] * w_norm_max + bias_abs_max (Cauchy-Schwarz; w_norm_max = max_n ||W[n]||_2 of the
 * dequantised weights, a_l2 from mi355x_sd_adaln_f8), |gelu(x)| <= |x|, so c_scale[m] = 1.1 * that bound / 448 cannot
 * overflow; e4m3 is a floating-point format, a scale that is ~10x loose costs precision only for elements ~100x below
 * the typical magnitude. ldc in bytes, % 8. */
int mi355x_sd_linear_f8_q(const void* A8, int lda, const float* a_scale, const float* a_l2, const void* W8,
                          const float* w_scale, float w_norm_max, void* C8, int ldc, float* c_scale, int M, int N, int K,
                          const float* bias, float bias_abs_max, int flags, void* stream);
/* bf16 rows -> e4m3 rows + per-row scale (attention output in front of the output projections, GELU output in front
 * of ff.net.2). Source row m lives at (m / x_rows_per_batch) * x_batch_stride + (m % x_rows_per_batch) * ldx
 * (x_rows_per_batch = 0: plain m * ldx); the output rows and scales are compact. */
int mi355x_sd_quantize_rows(const void* x, int64_t rows, int C, int ldx, int x_rows_per_batch, int64_t x_batch_stride,
                            void* y8, int ldy, float* y_scale, void* stream);

/* y = LayerNorm_noaffine(x) * (1 + scale[b]) + shift[b], b = row / rows_per_batch, scale/shift fp32 rows of stride ld_mod.
 * AdaLayerNormZero / AdaLayerNormContinuous (PPD/models/normalization.py:72-86, 190-202) and the Triton op
 * adaptive_layer_norm (paddlemix/triton_ops/triton_ops.py:981-1139). */
int mi355x_sd_adaln(const void* x, int rows, int C, int ldx, const float* scale, const float* shift, int ld_mod,
                    int rows_per_batch, float eps, void* y, int ldy, void* stream);
/* Element type of the modulation (gate / scale / shift) and affine (weight / bias) vectors of the _ex forms below.
 * MI355X_SD_MOD_ELEM = the build's 16-bit element type: what the REFERENCE's ops receive -- gate_msa / scale_mlp / shift_mlp are
 * chunks of a 16-bit linear output and weight / bias 16-bit parameters, all of x.dtype (paddlemix/triton_ops/triton_ops.py:777-786,
 * call sites PPD/models/simplified_sd3.py:62-76); ld_mod % 8 == 0 and 16-byte aligned vectors then. MI355X_SD_MOD_F32: fp32
 * vectors (ld_mod % 4 == 0), what this library's own SD3 / DiT programs keep them in. */
#define MI355X_SD_MOD_F32 0
#define MI355X_SD_MOD_ELEM 1
int mi355x_sd_adaln_ex(const void* x, int rows, int C, int ldx, const void* scale, const void* shift, int ld_mod, int mod_dtype,
                       int rows_per_batch, float eps, void* y, int ldy, void* stream);
/* PatchEmbed.proj operand (PPD/models/embeddings.py:148-155, 209-219): NCHW fp32 -> rows [B*(H/p)*(W/p), C*p*p] bf16,
 * columns ordered (c, py, px) like the flattened conv weight; and the inverse at the output (transformer_sd3.py:349-356):
 * rows [B*h*w, p*p*C] ordered (py, px, c) -> NCHW fp32. */
int mi355x_sd_patchify(const float* x_nchw, int B, int C, int H, int W, int patch, void* out, int ldo, void* stream);
int mi355x_sd_unpatchify(const void* x, int ldx, int B, int C, int H, int W, int patch, float* out_nchw, void* stream);

/* 3x3 convolution, padding 1 (or bottom/right only with MI355X_SD_PAD_BR), stride 1|2, as an implicit GEMM over an NHWC source [B][Hs][Ws][ldx>=Cin];
 * `upsample` = 1 folds F.interpolate(scale_factor=2, mode="nearest") (PPD/models/resnet.py:169-218) into the
 * gather.  W is [Cout][3][3][Cin].  Output rows = B*Ho*Wo with Ho = ((Hs<<upsample) + 2 - 3)/stride + 1
 * (PAD_BR: ((Hs + 1 - 3)/2 + 1).
 * Replaces LoRACompatibleConv.forward (lora.py:364-377) as used by ResnetBlock2D (resnet.py:770,798, temb add
 * :772-784 via rowbias), Downsample2D (:271-294) and Upsample2D. */
int mi355x_sd_conv3x3(const void* X, int ldx, int B, int Hs, int Ws, int Cin, int stride, int upsample,
                      const void* W, void* C, int ldc, int Cout,
                      const float* bias, const float* rowbias, int ld_rowbias,
                      const void* R, int ldr, float out_scale, int flags, void* ws, size_t ws_bytes, void* stream);

/* out = softmax(q k^T * scale + bias) v, layouts q [B,Sq,H,D], k/v [B,Skv,H,D], out [B,Sq,H,D] with explicit
 * batch (bs) and token (ts) strides in elements; bias optional fp32 additive mask addressed
 * b*bias_bs + h*bias_hs + q*bias_qs + kv (0 strides broadcast).  D % 8 == 0, D <= 160.
 * A query row whose keys are ALL masked with -inf has no softmax: its output row is 0 (torch's sdpa gives NaN there).
 * Replaces scaled_dot_product_attention_ (PPD/patches/paddle_patch.py:414-529) and the body of
 * AttnProcessor.__call__ / get_attention_scores (PPD/models/attention_processor.py:673-735, 552-586). */
int mi355x_sd_sdpa(const void* q, const void* k, const void* v, const float* bias, void* out,
                   int B, int H, int Sq, int Skv, int D,
                   int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts, int64_t o_bs, int o_ts,
                   int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale, void* stream);

/* out += out_scale * softmax(q k^T * scale + bias) v  -- same layouts as mi355x_sd_sdpa, `out` already holding the result of
 * a first attention over another key set. IPAdapterAttnProcessor.__call__ (PPD/models/attention_processor.py:1819-1901):
 * hidden = attn(q, to_k(text), to_v(text)) + self.scale * attn(q, to_k_ip(image tokens), to_v_ip(image tokens)) (:1871-1886). */
/* mi355x_sd_sdpa with flags. MI355X_SD_SDPA_LOG2: the caller has folded scale * log2(e) into the queries (e.g. into the to_q
 * weights), so q.k IS the base-2 exponent: out = softmax_2(q k^T) v with softmax_2(x) = 2^x / sum 2^x; `scale` is ignored, no mask,
 * D == 64. Saves the multiply-add per score in front of every exponential (profiles/HISTORY.md section 5). */
#define MI355X_SD_SDPA_LOG2 1
int mi355x_sd_sdpa_ex(const void* q, const void* k, const void* v, const float* bias, void* out, int B, int H, int Sq, int Skv, int D,
                      int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts, int64_t o_bs, int o_ts,
                      int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale, int flags, void* stream);
int mi355x_sd_sdpa_accum(const void* q, const void* k, const void* v, const float* bias, void* out,
                   int B, int H, int Sq, int Skv, int D,
                   int64_t q_bs, int q_ts, int64_t k_bs, int k_ts, int64_t v_bs, int v_ts, int64_t o_bs, int o_ts,
                   int64_t bias_bs, int64_t bias_hs, int64_t bias_qs, float scale, float out_scale, void* stream);

/* GroupNorm statistics -> scale_shift[B][2][C] fp32 (scale = gamma*rstd, shift = beta - mean*scale); x is
 * [B][HW][ldx>=C].  `workspace` needs mi355x_sd_groupnorm_workspace_floats(B,HW,C) floats.
 * paddle.nn.GroupNorm as used at PPD/models/resnet.py:739,789; transformer_2d.py:359; unet_2d_condition.py:1194. */
int mi355x_sd_groupnorm_workspace_floats(int B, int HW, int C);
int mi355x_sd_groupnorm_stats(const void* x, int B, int HW, int C, int ldx, int groups, float eps,
                              const float* gamma, const float* beta, float* workspace, float* scale_shift,
                              void* stream);
/* GroupNorm (+SiLU when silu != 0) of 16-bit rows in ONE launch: x, y [B][HW][ld >= C]. Only where a (batch, group) chunk fits a
 * block's registers: HW * (C / groups) * 2 bytes <= 96 KiB and C / groups even (mi355x_sd_groupnorm_act_fits returns 1; else
 * MI355X_SD_ERR_UNSUPPORTED -- use the stats + scale_shift_act pair). Same arithmetic as the pair (fp32 sums per thread, double
 * mean / variance, y = x * (gamma * rstd) + (beta - mean * gamma * rstd)); the summation order differs, so results agree with the
 * pair to fp32 rounding of the statistics, not bit for bit. */
int mi355x_sd_groupnorm_act_fits(int HW, int C, int groups);
int mi355x_sd_groupnorm_act(const void* x, int B, int HW, int C, int ldx, int groups, float eps, const float* gamma,
                            const float* beta, int silu, void* y, int ldy, void* stream);
/* y = act(x*scale[b][c] + shift[b][c]), act = SiLU when silu != 0 (the fused GN+SiLU of resnet.py:739-741). */
int mi355x_sd_scale_shift_act(const void* x, int B, int HW, int C, int ldx, const float* scale_shift, int silu,
                              void* y, int ldy, void* stream);
/* Row LayerNorm with optional affine (PPD/models/attention.py:397,442,463). C <= 2560. */
int mi355x_sd_layernorm(const void* x, int rows, int C, int ldx, const float* gamma, const float* beta, float eps,
                        void* y, int ldy, void* stream);
/* The same three with x_f32 != 0: x is fp32 rows (ldx in fp32 elements) -- the norms are where the fp32 residual stream
 * becomes a 16-bit MFMA operand. scale_shift_act_ex can also emit raw16 (NULL: none) = the 16-bit rounding of the raw x
 * rows in the same pass: the operand of the resnet's conv_shortcut GEMM (resnet.py:797-798). */
int mi355x_sd_groupnorm_stats_ex(const void* x, int B, int HW, int C, int ldx, int groups, float eps,
                                 const float* gamma, const float* beta, float* workspace, float* scale_shift,
                                 int x_f32, void* stream);
int mi355x_sd_scale_shift_act_ex(const void* x, int B, int HW, int C, int ldx, const float* scale_shift, int silu,
                                 void* y, int ldy, int x_f32, void* raw16, int ld_raw, void* stream);
int mi355x_sd_layernorm_ex(const void* x, int rows, int C, int ldx, const float* gamma, const float* beta, float eps,
                           void* y, int ldy, int x_f32, void* stream);
/* y (16-bit rows) = x (fp32 rows): operand copies of the fp32 residual stream (inputs of Downsample2D / Upsample2D convs). */
int mi355x_sd_cast_rows(const float* x, int ldx, void* y, int ldy, int64_t rows, int C, void* stream);

/* ---- the reference's fused custom ops, with THEIR signatures (seam B4; paddlemix/triton_ops/triton_ops.py) ----
 * fused_adaLN_scale_residual(x, mha_out, gate_msa, scale_mlp, shift_mlp, weight, bias, epsilon) -> (resi_out, adaLN_out)
 * (triton_ops.py:758-920; unfused definition :842-847): resi_out = mha_out * gate[b] + x, adaLN_out = layer_norm(resi_out, weight,
 * bias, eps) * (1 + scale[b]) + shift[b], b = row / rows_per_batch. x, mha_out, resi_out, adaLN_out: 16-bit rows [rows][ld >= C];
 * gate / scale / shift: fp32 [rows / rows_per_batch][ld_mod >= C]; weight / bias fp32 [C] or NULL. C % 8 == 0, C <= 4096.
 * (fp32 vectors: this library's own convention; the reference passes them in x.dtype -- use the _ex form below for a one-for-one swap) */
int mi355x_sd_fused_adaln_scale_residual(const void* x, int ldx, const void* mha_out, int ld_mha, const float* gate_msa,
                                         const float* scale_mlp, const float* shift_mlp, int ld_mod, int rows_per_batch,
                                         const float* weight, const float* bias, float epsilon, int rows, int C,
                                         void* resi_out, int ld_resi, void* adaln_out, int ld_out, void* stream);
/* The one-for-one form: gate / scale / shift / weight / bias in mod_dtype (MI355X_SD_MOD_ELEM = the tensors exactly as the reference
 * hands them to fused_adaLN_scale_residual: all of x.dtype). Arithmetic in fp32 either way. */
int mi355x_sd_fused_adaln_scale_residual_ex(const void* x, int ldx, const void* mha_out, int ld_mha, const void* gate_msa,
                                            const void* scale_mlp, const void* shift_mlp, int ld_mod, int mod_dtype,
                                            int rows_per_batch, const void* weight, const void* bias, float epsilon, int rows,
                                            int C, void* resi_out, int ld_resi, void* adaln_out, int ld_out, void* stream);
/* split_concat(x [B,S1,3C], y [B,S2,3C]) -> q, k, v, each [B, S1+S2, C]: chunk i of x followed by chunk i of y along the sequence
 * (triton_ops.py:1692-1752); dense 16-bit tensors, C % 8 == 0. */
int mi355x_sd_split_concat(const void* x, const void* y, void* q_out, void* k_out, void* v_out, int B, int S1, int S2, int C,
                           void* stream);

/* get_timestep_embedding (PPD/models/embeddings.py:26-64) in fp32, written as bf16 to
 * out[(i/group)*ldo + (i%group)*dim + j] for i < n, timestep t[i % t_count] (device fp32). */
int mi355x_sd_timestep_embedding(const float* t, int t_count, int n, int dim, int group, int flip_sin_to_cos,
                                 float freq_shift, float scale, float max_period, void* out, int ldo, void* stream);
int mi355x_sd_silu(const void* x, void* y, int64_t n, int in_f32, int out_f32, void* stream);

/* conv_in (PPD/models/unet_2d_condition.py:1064): x NCHW fp32, optional device scalar in_scale (the scheduler's
 * scale_model_input), w [9*Cin][Cout] bf16, y NHWC bf16. */
int mi355x_sd_conv_in3x3(const float* x_nchw, const float* in_scale, const void* w, const float* bias, void* y,
                         int B, int Cin, int H, int W, int Cout, int ldy, void* stream);
/* out_f32 != 0: y is NHWC fp32 (start of the fp32 residual stream) */
int mi355x_sd_conv_in3x3_ex(const float* x_nchw, const float* in_scale, const void* w, const float* bias, void* y,
                            int B, int Cin, int H, int W, int Cout, int ldy, int out_f32, void* stream);
/* conv_out (unet_2d_condition.py:1196): x NHWC bf16, w [Cout<=4][3][3][Cin] bf16, y NCHW fp32. */
int mi355x_sd_conv_out3x3(const void* x, int ldx, const void* w, const float* bias, float* y_nchw,
                          int B, int Cin, int H, int W, int Cout, void* stream);
int mi355x_sd_copy_rows(const void* x, int ldx, void* y, int ldy, int64_t rows, int C, void* stream);

/* ControlNet residual inputs of UNet2DConditionModel.forward (down_block_additional_residuals /
 * mid_block_additional_residual, PPD/models/unet_2d_condition.py:1121-1132, 1151-1155): x[b*HW + p][c] += r[b][c][p] in place
 * on a bf16 NHWC row view (row stride ldx; C % 8 == 0), r NCHW fp32 as the reference passes it. */
int mi355x_sd_add_nchw(void* x, int ldx, const float* r_nchw, int B, int C, int64_t HW, void* stream);
int mi355x_sd_add_nchw_ex(void* x, int ldx, const float* r_nchw, int B, int C, int64_t HW, int x_f32, void* stream);

/* FreeU (apply_freeu / fourier_filter, PPD/utils/paddle_utils.py:259-313; ABI 22) in place on a concat buffer of the U-Net's up path:
 * cat is B*H*W rows of Cx backbone columns followed by Cs skip columns, row stride ld elements (bf16, or fp32 when elem_f32 != 0).
 *   columns [0, Cx / 2)    *= b
 *   columns [Cx, Cx + Cs)  <- the Fourier filter with threshold 1 and scale s of every (batch, channel) plane [H][W]: the four shifted
 *                             FFT bins ky, kx in {-1, 0} scaled by s, i.e. with ty = 2 pi y / H, tx = 2 pi x / W and <.> the plane's mean
 *                             out = x + (s - 1) (<x> + sum over phi in {ty, tx, ty + tx} of <x cos phi> cos phi + <x sin phi> sin phi)
 *   columns [Cx / 2, Cx) and [Cx + Cs, ld) are not written.
 * fp32 arithmetic, one rounding per stored element, no atomics: two runs give the same bits. `workspace` needs
 * mi355x_sd_freeu_workspace_floats(B, H, W, Cs) floats (0 for arguments the call would refuse), 16-byte aligned.
 * MI355X_SD_ERR_INVALID: a null pointer, B < 1, H < 2, W < 2, Cx < 0, Cs < 1, ld < Cx + Cs, cat or the row stride in bytes not a
 * multiple of 16, b or s not finite. MI355X_SD_ERR_UNSUPPORTED: W > 4096 or B > 65535. */
int64_t mi355x_sd_freeu_workspace_floats(int B, int H, int W, int Cs);
int mi355x_sd_freeu(void* cat, int64_t ld, int B, int H, int W, int Cx, int Cs, float b, float s, int elem_f32, float* workspace,
                    void* stream);

/* ---- T2I-Adapter (PPD/models/adapter.py; ABI 23): the three layers the adapter has and no other model here does. Its convolutions
 * are mi355x_sd_conv3x3 and mi355x_sd_linear. ----
 * nn.PixelUnshuffle(r) (adapter.py:306, :356, :484) fused with the NCHW fp32 -> NHWC bf16 change the next convolution needs:
 *   y[(b*(H/r) + i)*(W/r) + j][c*r*r + dy*r + dx] = bf16(x[b][c][i*r + dy][j*r + dx])        one rounding per element
 * x NCHW fp32 [B][C][H][W]; y rows of ldy bf16 elements; columns [C*r*r, ldy) are not written. r % 8 == 0 with x 16-byte aligned
 * stores 16 bytes per thread (the adapter's r = 8, 16); any other r goes element by element.
 * MI355X_SD_ERR_INVALID: a null pointer, B, C, H, W or r < 1, H % r or W % r nonzero, ldy < C*r*r, ldy % 8 nonzero, y not 16-byte
 * aligned. MI355X_SD_ERR_UNSUPPORTED: C*r*r >= 2^31. */
int mi355x_sd_pixel_unshuffle(const float* x_nchw, int B, int C, int H, int W, int r, void* y, int ldy, void* stream);
/* nn.AvgPool2D(kernel_size=2, stride=2, ceil_mode=True) (adapter.py:411, :537) on NHWC bf16 rows: x [B*H*W][ldx] -> y
 * [B*ceil(H/2)*ceil(W/2)][ldy], C channels. A window that hangs over the bottom or right edge averages its in-bounds elements only
 * (Paddle's exclusive=True default). fp32 sum in the order (0,0), (0,1), (1,0), (1,1), one multiply by 1, 1/2 or 1/4, one rounding.
 * MI355X_SD_ERR_INVALID: a null pointer, B, H, W or C < 1, ldx < C, ldy < C. MI355X_SD_ERR_UNSUPPORTED: C, ldx or ldy not a
 * multiple of 8, x or y not 16-byte aligned. */
int mi355x_sd_avgpool2(const void* x, int ldx, int B, int H, int W, int C, void* y, int ldy, void* stream);
/* nn.ReLU (adapter.py:450, :571): y[row][c] = max(x[row][c], 0) on `rows` bf16 rows of C elements (row strides ldx, ldy); y == x (in
 * place) is allowed, any other overlap is not. C, ldx, ldy multiples of 8 and both pointers 16-byte aligned: 16 bytes per thread.
 * MI355X_SD_ERR_INVALID: a null pointer, rows < 1, C < 1, ldx < C, ldy < C. */
int mi355x_sd_relu(const void* x, int ldx, void* y, int ldy, int64_t rows, int C, void* stream);

/* DiagonalGaussianDistribution (PPD/models/vae.py:744-763, built by AutoencoderKL.encode, autoencoder_kl.py:266-283) from
 * the encoder's moments held as fp32 rows [B*HW][ld >= 2L] (channels mean_0..L-1, logvar_0..L-1): writes NCHW fp32
 * mean ( = .mode()), logvar clipped to [-30, 20] and -- sample_nchw != NULL -- (mean + exp(0.5 logvar) * noise) * out_scale
 * ( = .sample() with the caller's noise, times the pipelines' vae.config.scaling_factor; noise NULL: mean * out_scale). */
int mi355x_sd_latent_dist(const float* moments, int ld, int B, int L, int64_t HW, const float* noise_nchw, float out_scale,
                          float* mean_nchw, float* logvar_nchw, float* sample_nchw, void* stream);

/* ---- CLIP text encoder (PPD/transformers/clip/modeling.py) ----
 * CLIPTextEmbeddings.forward (:214-231): out[i][:] = bf16(token_table[ids[i]] + position_table[i % seq_len]); tables bf16
 * [V][D] / [P][D], ids int32 in device memory (range-checked by the caller), D % 8 == 0. position_table may be NULL
 * (token embedding only: T5Stack.embed_tokens, PPD/transformers/t5/modeling.py:981-983). */
int mi355x_sd_embed_tokens(const int32_t* ids, int64_t n_tokens, int seq_len, const void* token_table,
                           const void* position_table, int D, void* out, int ldo, void* stream);
/* y = act(x) on n bf16 elements (n % 8 == 0): kind 0 quick_gelu (x sigmoid(1.702 x), CLIPMLP :338-350 with
 * hidden_act="quick_gelu"), 1 gelu (erf), 2 silu. The rest of CLIPEncoderLayer (:353-400) is mi355x_sd_layernorm,
 * mi355x_sd_linear (bias / residual epilogues) and mi355x_sd_sdpa with the causal mask as its additive bias. */
int mi355x_sd_activation(const void* x, void* y, int64_t n, int kind, void* stream);

/* ---- T5 encoder (the third text encoder of SD3; PPD/transformers/t5/modeling.py) ----
 * T5LayerNorm (:86-108): y = weight * x * rsqrt(mean(x^2) + eps) -- RMS norm, fp32 statistics, no bias; C <= 4096. */
int mi355x_sd_rmsnorm(const void* x, int rows, int C, int ldx, const float* weight, float eps, void* y, int ldy,
                      void* stream);
/* T5DenseGatedActDense (:164-167) on the fused [wi_0 | wi_1] projection x [rows, 2F]: y[r][j] = act(x[r][j]) * x[r][F+j];
 * kind 0 quick_gelu, 1 gelu (erf), 2 silu, 3 gelu_new (tanh approximation; T5 v1.1 "gated-gelu"). F % 8 == 0.
 * T5Attention (:308-424) is mi355x_sd_linear (no bias) + mi355x_sd_sdpa with scale 1.0 and the relative position bias
 * [1, heads, S, S] (compute_bias :293-306) as the additive mask. */
int mi355x_sd_gated_activation(const void* x, int ldx, void* y, int ldy, int64_t rows, int F, int kind, void* stream);

/* ---- AutoencoderKL decoder (PPD/models/autoencoder_kl.py:288-333, PPD/models/vae.py:182-343) ----
 * post_quant_conv (autoencoder_kl.py:121,292-293): 1x1 convolution of a small NCHW fp32 tensor, Cin, Cout <= 16,
 * y[b,co,p] = bias[co] + sum_ci w[co][ci] * bf16(x[b,ci,p] * in_scale); in_scale = 1 / scaling_factor of the calling
 * pipeline (pipeline_stable_diffusion.py:911). w bf16 [Cout][Cin]. */
int mi355x_sd_conv1x1_nchw(const float* x_nchw, float in_scale, const void* w, const float* bias, float* y_nchw,
                           int B, int Cin, int Cout, int64_t HW, void* stream);
/* ---- tiled AutoencoderKL (PPD/models/autoencoder_kl.py:334-446 tiled_encode / tiled_decode, blend_v / blend_h) ----
 * tile_gather: copies a regular grid of equal windows of an fp32 NCHW tensor [B, C, H, W] into a stack of contiguous NCHW images
 * [count, C, win_h, win_w] (the input batch of one tile plan). Window (iy, ix) of image b starts at (y0 + iy * stride_y,
 * x0 + ix * stride_x) and is stack image n = (b * ny + iy) * nx + ix; the call writes images first <= n < first + count to dst[0..).
 * Every window must lie inside the source. Rows that keep 16-byte alignment (W, x0, stride_x, win_w multiples of 4) move as 16-byte
 * vectors. */
int mi355x_sd_tile_gather(const float* src_nchw, int B, int C, int H, int W, int y0, int x0, int stride_y, int stride_x, int ny,
                          int nx, int win_h, int win_w, int64_t first, int64_t count, float* dst, void* stream);
/* tile_blend: the seam blend, crop and concatenation of the reference's tiled_decode / tiled_encode in one pass that writes every
 * element of out [B, C, H, W] exactly once. Tile (i, j) covers the output from (i * lim, j * lim) and has min(S, H - i * lim) rows and
 * min(S, W - j * lim) columns (ny = ceil(H / lim), nx = ceil(W / lim): derived here, not read from a table). The first
 * e = min(extent of the neighbour, own extent, ext) rows of a tile are blended with the last e rows of the tile above,
 * b[p] = a[Ea - e + p] * (1 - p / e) + b[p] * (p / e), then the first columns with the tile to the left, in the reference's order and
 * rounding (the closed form of its sequential in-place algorithm, bit for bit in fp32: two rounded products and a rounded sum per
 * lerp, no fma; needs ext <= lim <= S so that a blend reads rows the neighbour's own blend did not touch); everything else is a copy.
 * tile_ptrs: DEVICE array of B * ny * nx pointers, [(b * ny + i) * nx + j] = element (channel 0, row 0, column 0) of tile (i, j) of
 * image b. Inside a tile of eh x ew, element (c, y, x) lies at c * (t_chan_plane * eh * ew + t_chan) + (y * ew + x) * t_col floats:
 * (1, 0, 1) = contiguous planes (the decoder's NCHW images), (0, 1, ld) = token-major rows [eh * ew][ld] (the encoder's moments).
 * The output takes plain element strides (image, channel, row, column). With unit column strides and W, S, lim, ext multiples of 4
 * the kernel moves 16-byte vectors. */
int mi355x_sd_tile_blend(const void* tile_ptrs, int B, int C, int H, int W, int S, int lim, int ext, int ny, int nx,
                         int64_t t_chan_plane, int64_t t_chan, int64_t t_col, float* out, int64_t o_img, int64_t o_chan, int64_t o_row,
                         int64_t o_col, void* stream);
/* y[r][0..n) = softmax(x[r][0..n)), x fp32 (scale already applied), y bf16; n % 4 == 0. The VAE mid-block attention
 * (one head of width C = 512: Attention(..., heads = C // C), unet_2d_blocks.py:606-619; get_attention_scores with
 * upcast_softmax, attention_processor.py:552-586) runs as linear(Q K^T, OUT_F32) -> softmax_rows -> linear(P V). */
int mi355x_sd_softmax_rows(const float* x, int64_t ldx, void* y, int64_t ldy, int64_t rows, int n, void* stream);
/* out = coef[0]*x + coef[1]*y on fp32 latents, coef in device memory: the linear latent update every
 * epsilon-prediction scheduler step reduces to (PPD/schedulers/scheduling_euler_discrete.py:438-473,
 * scheduling_ddim.py:410-457 with eta = 0). */
int mi355x_sd_axpby(const float* x, const float* y, float* out, const float* coef, int64_t n, void* stream);
/* The same update with the classifier-free-guidance combine folded in (pipeline_stable_diffusion.py:882-891):
 * out = coef[0]*x + coef[1]*(eps_uncond + guidance_scale * (eps_text - eps_uncond)); eps_* = the two batch halves of the
 * UNet output. */
int mi355x_sd_cfg_axpby(const float* x, const float* eps_uncond, const float* eps_text, float* out, const float* coef,
                        float guidance_scale, int64_t n, void* stream);
/* The same update with the guidance rescale folded in as well (rescale_noise_cfg, pipeline_stable_diffusion.py:69-80; the
 * `guidance_rescale` of the SD / SDXL pipelines, used with v-prediction and zero-terminal-SNR checkpoints). Per sample s of `batch`,
 * over its per_sample = C * H * W elements: c = eps_uncond + guidance_scale * (eps_text - eps_uncond), r[s] = std(eps_text[s]) / std(c[s])
 * (the unbiased estimator; each variance by two passes, mean first, then the squared deviations),
 * out = coef[0]*x + coef[1] * c * (guidance_rescale * r[s] + 1 - guidance_rescale). One launch, one block per sample, no scratch; the
 * reductions are fixed trees without atomics, so equal inputs give equal bits. A sample of zero variance divides as the reference
 * does (inf / NaN): no epsilon is added. out may be x itself; out overlapping x in any other way, or eps_uncond / eps_text at all, is
 * MI355X_SD_ERR_INVALID, as are batch <= 0 and per_sample < 2 (the estimator divides by per_sample - 1). */
int mi355x_sd_cfg_rescale_axpby(const float* x, const float* eps_uncond, const float* eps_text, float* out, const float* coef,
                                float guidance_scale, float guidance_rescale, int batch, int64_t per_sample, void* stream);

/* One step of DPM-Solver multistep sampling (DPMSolverMultistepScheduler: dpmsolver++ / dpmsolver, solver_order 1 and 2, midpoint /
 * heun) in one launch: guidance combine, guidance rescale, convert_model_output, the multistep update and its history. coef is 5
 * fp32 values (p, q, A, B, D) in device memory, read by the kernel (DPMSolverMultistepScheduler.multistep_coefficients), so a
 * captured graph replays with another row. Per element, with e the guided model output (c of mi355x_sd_cfg_axpby; with
 * guidance_rescale > 0 times the per-sample factor of mi355x_sd_cfg_rescale_axpby, same statistics, one block per sample):
 *   m0 = p*x + q*e  -> m_out,      out = A*x + B*m0 + D*(m0 - m_prev)
 * eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 * coef[4] == 0 (a first-order step) : m_prev is NOT read, so the uninitialised history of a fresh loop is harmless; it must still be
 * a valid non-null pointer (a captured graph cannot change it between replays).
 * Aliasing: out may be x itself and m_out may be m_prev itself (one history buffer); each element is read and written by the same
 * lane in the last pass only. Every other overlap among out, m_out, the inputs and coef is MI355X_SD_ERR_INVALID before any launch, as
 * are a null x, eps_uncond, m_prev, out, m_out or coef, batch <= 0, per_sample < 1, and per_sample < 2 with guidance_rescale > 0. */
int mi355x_sd_multistep_update(const float* x, const float* eps_uncond, const float* eps_text, const float* m_prev, float* out,
                               float* m_out, const float* coef, float guidance_scale, float guidance_rescale, int batch,
                               int64_t per_sample, void* stream);

/* One step of UniPC sampling (UniPCMultistepScheduler: solver_order 1-3, bh1 / bh2, predict_x0 or not) in one launch: guidance
 * combine, guidance rescale, convert_model_output, the B(h) corrector, the B(h) predictor, last_sample and the history shift.
 * State the caller owns for the duration of a loop, fp32 device memory: `last`, one plane of batch * per_sample floats, and `hist`,
 * `order` such planes, plane 0 the newest converted model output. Per element, with e the guided (and rescaled) model output as in
 * mi355x_sd_multistep_update, L = last and h1, h2, h3 = planes 0, 1, 2 before this call:
 *   m_t = p*x + q*e
 *   x_c = Ac*L + Bc*h1 + C2*(h2 - h1) + C3*(h3 - h1) + Ct*(m_t - h1)   if corr != 0, else x_c = x          -> last
 *   out = Ap*x_c + Bp*m_t + D1*(h1 - m_t) + D2*(h2 - m_t)
 *   plane[k] <- plane[k-1] for k = order-1 .. 1, plane[0] <- m_t
 * Rules:
 *  - coef is 12 fp32 values (p, q, Ac, Bc, C2, C3, Ct, Ap, Bp, D1, D2, corr) in device memory, 16-byte aligned, read by the kernel
 *    (UniPCMultistepScheduler.unipc_coefficients): every pointer stays fixed from step to step and a captured graph of one node
 *    replays a whole loop with only the row changing.
 *  - eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 *  - a term whose coefficient is 0.0 is not formed and its operand does not enter the arithmetic: L, each plane inside a difference,
 *    the whole corrector when corr == 0. These are wave-uniform branches on the values of the row. The uninitialised last / hist of a
 *    fresh loop, or of an img2img start inside the schedule, therefore never reach out. Planes at or past `order` are never touched.
 *  - the shift may copy uninitialised planes, bit for bit; that is harmless.
 *  - operation order: each difference is formed first and then multiplied; the corrector's terms are summed left to right as written,
 *    the predictor's likewise; which product contracts into which sum is the compiler's choice, as in mi355x_sd_multistep_update.
 *  - two launches on equal inputs give equal bits (no atomics; the rescale's sums are the fixed trees of mi355x_sd_cfg_rescale_axpby).
 *  - two forms: guidance_rescale > 0 with eps_text runs one 1024-thread block per sample (the statistics passes of
 *    mi355x_sd_cfg_rescale_axpby; a sample of <= 32768 elements stays in registers, larger ones are re-read); otherwise a grid-stride
 *    elementwise kernel with 16-byte vectors when every pointer and plane is 16-byte aligned, and a scalar tail. No scratch memory.
 *  - aliasing: out may be x itself. Any other overlap among out, last, hist, the inputs and coef is MI355X_SD_ERR_INVALID before any
 *    launch, as are a null pointer (except eps_text), a coef that is not 16-byte aligned, order outside 1..3, batch <= 0,
 *    per_sample < 1, and per_sample < 2 with guidance_rescale > 0. */
int mi355x_sd_unipc_update(const float* x, const float* eps_uncond, const float* eps_text, float* last, float* hist, int order,
                           float* out, const float* coef, float guidance_scale, float guidance_rescale, int batch,
                           int64_t per_sample, void* stream);

/* One step of ancestral sampling (EulerAncestralDiscreteScheduler, "Euler a": a deterministic move plus fresh noise every step) in one
 * launch: guidance combine, guidance rescale and the update. `noise` is a plane of batch * per_sample fp32 values z ~ N(0, I) the
 * caller draws once per step; the kernel draws nothing. Per element, with e the guided (and rescaled) model output as in
 * mi355x_sd_multistep_update:
 *   out = a*x + b*e
 *   out = out + c*noise        only if c != 0
 * Rules:
 *  - coef is 3 fp32 values (a, b, c) in device memory, read by the kernel (EulerAncestralDiscreteScheduler.ancestral_coefficients):
 *    a captured graph of one node replays a whole loop with only the row changing and the noise plane rewritten in place.
 *  - eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 *  - c == 0.0 (the last row of every schedule, where sigma_up = 0) is a wave-uniform branch on the device value: noise is NOT
 *    dereferenced, so a stale or NaN plane cannot reach the final latents. The entry cannot see a device value, so it accepts
 *    noise == NULL; that is valid ONLY for a row the caller knows to have c == 0. A caller that replays one graph passes a real plane.
 *  - operation order: as written above; which product contracts into which sum is the compiler's choice, as in
 *    mi355x_sd_multistep_update.
 *  - two launches on equal inputs give equal bits (no atomics; the rescale's sums are the fixed trees of mi355x_sd_cfg_rescale_axpby).
 *  - two forms: guidance_rescale > 0 with eps_text runs one 1024-thread block per sample (the statistics passes of
 *    mi355x_sd_cfg_rescale_axpby; a sample of <= 32768 elements stays in registers, larger ones are re-read); otherwise a grid-stride
 *    elementwise kernel with 16-byte vectors when every pointer is 16-byte aligned, and a scalar tail. No scratch memory.
 *  - aliasing: out may be x itself. Any other overlap of out with x, eps_uncond, eps_text, noise or coef is MI355X_SD_ERR_INVALID
 *    before any launch, as are a null x, eps_uncond, out or coef, batch <= 0, per_sample < 1, and per_sample < 2 with
 *    guidance_rescale > 0. */
int mi355x_sd_ancestral_update(const float* x, const float* eps_uncond, const float* eps_text, const float* noise, float* out,
                               const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                               void* stream);

/* One model evaluation of a two-stage, second-order step (HeunDiscreteScheduler, "Heun": an Euler step, then Heun's correction from
 * the same start; 2n - 1 evaluations for n steps) in one launch: guidance combine, guidance rescale, the derivative and the update.
 * `sample` (S) and `deriv` (D) are two caller-owned planes of batch * per_sample fp32 values that hold the step's state between
 * its two launches. Per element, with e the guided (and rescaled) model output as in mi355x_sd_multistep_update:
 *   d = p*x + q*e                                  p == 0: d = q*e, the product with x is not formed
 *   second == 0:  out = x + h*d                    S <- x (bit copy), D <- d; S and D are NOT read
 *   second != 0:  out = S + h*(g*D + d)            g == 0: D is NOT read; S and D are NOT written
 * Rules:
 *  - coef is 5 fp32 values (p, q, h, g, second) in device memory, read by the kernel (HeunDiscreteScheduler.heun_coefficients): a
 *    captured graph of one node replays a whole loop, both stages, with only the row changing and S / D at fixed addresses.
 *  - eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 *  - second, p == 0 and g == 0 are wave-uniform branches on the device values. State a stage does not need is not dereferenced:
 *    neither plane needs initialising before the first stage-1 launch, and stale or NaN contents cannot reach out. g weights the
 *    parked derivative: Heun's average uses 1 (h carries the 1/2); a midpoint method uses 0 and never reads D.
 *  - operation order: as written above; which product contracts into which sum is the compiler's choice, as in
 *    mi355x_sd_multistep_update.
 *  - two launches on equal inputs give equal bits (no atomics; the rescale's sums are the fixed trees of mi355x_sd_cfg_rescale_axpby).
 *  - two forms: guidance_rescale > 0 with eps_text runs one 1024-thread block per sample (the statistics passes of
 *    mi355x_sd_cfg_rescale_axpby; a sample of <= 32768 elements stays in registers, larger ones are re-read); otherwise a grid-stride
 *    elementwise kernel with 16-byte vectors when x, sample, deriv, out and the eps planes are 16-byte aligned, and a scalar tail.
 *    No scratch memory.
 *  - aliasing: out may be x itself. Any other overlap of out, sample or deriv with each other, x, eps_uncond, eps_text or coef is
 *    MI355X_SD_ERR_INVALID before any launch, as are a null x, eps_uncond, sample, deriv, out or coef, batch <= 0, per_sample < 1,
 *    and per_sample < 2 with guidance_rescale > 0. */
int mi355x_sd_heun_update(const float* x, const float* eps_uncond, const float* eps_text, float* sample, float* deriv, float* out,
                          const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                          void* stream);

/* One model evaluation of a two-stage midpoint step (KDPM2DiscreteScheduler, "DPM2": an Euler step to the midpoint sigma, then the whole
 * step from the same start with the derivative found there; KDPM2AncestralDiscreteScheduler, "DPM2 a": the same, ending at sigma_down
 * and adding noise of sigma_up; 2n - 1 evaluations for n steps) in one launch: guidance combine, guidance rescale, the derivative and
 * the update. `sample` (S) is one caller-owned plane of batch * per_sample fp32 values that holds the step's start between its two
 * launches; `noise` (z) is the caller's N(0, I) plane for this evaluation (the library draws nothing). Per element, with e the guided
 * (and rescaled) model output as in mi355x_sd_multistep_update:
 *   d = p*x + q*e                                  p == 0: d = q*e, the product with x is not formed
 *   second == 0:  out = x + h*d                    S <- x (bit copy); S and noise are NOT read
 *   second != 0:  out = S + h*d [+ c*z]            c == 0: the term is not formed and noise is NOT read; S is NOT written
 * Rules:
 *  - coef is 5 fp32 values (p, q, h, c, second) in device memory, read by the kernel (dpm2_coefficients of either scheduler): a
 *    captured graph of one node replays a whole loop, both stages, with only the row and the contents of noise changing and S at a
 *    fixed address.
 *  - eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 *  - second, p == 0 and c == 0 are wave-uniform branches on the device values. State a stage does not need is not dereferenced: S
 *    needs no initialising before the first stage-1 launch, and stale or NaN contents of S or noise cannot reach out where the row
 *    does not use them. noise is read by a stage-2 row with c != 0 only (every stage-2 row of DPM2 a; no row of DPM2). The DEVICE
 *    value decides: noise == NULL is accepted for a row the caller knows reads none, as in mi355x_sd_ancestral_update, and a host
 *    that replays one captured launch over both kinds of row keeps passing its plane.
 *  - operation order: as written above, the noise term added last; which product contracts into which sum is the compiler's choice,
 *    as in mi355x_sd_multistep_update.
 *  - two launches on equal inputs give equal bits (no atomics; the rescale's sums are the fixed trees of mi355x_sd_cfg_rescale_axpby).
 *  - two forms: guidance_rescale > 0 with eps_text runs one 1024-thread block per sample (the statistics passes of
 *    mi355x_sd_cfg_rescale_axpby; a sample of <= 32768 elements stays in registers, larger ones are re-read); otherwise a grid-stride
 *    elementwise kernel with 16-byte vectors when x, noise (NULL counts as aligned), sample, out and the eps planes are 16-byte
 *    aligned, and a scalar tail. No scratch memory.
 *  - aliasing: out may be x itself. Any other overlap of out or sample with each other, x, eps_uncond, eps_text, noise or coef is
 *    MI355X_SD_ERR_INVALID before any launch, as are a null x, eps_uncond, sample, out or coef, batch <= 0, per_sample < 1, and
 *    per_sample < 2 with guidance_rescale > 0. */
int mi355x_sd_dpm2_update(const float* x, const float* eps_uncond, const float* eps_text, const float* noise, float* sample, float* out,
                          const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                          void* stream);

/* One model evaluation of PLMS sampling (PNDMScheduler with skip_prk_steps, the scheduler of the SD-1.x checkpoints: a linear multistep
 * method over up to four model outputs; n steps are n + 1 evaluations, the second of which averages two outputs and steps again from
 * the loop's first sample) in one launch: guidance combine, guidance rescale, the history combination, the update, the history and
 * the parked sample. `park` (P) is one caller-owned plane of batch * per_sample fp32 values; `hist` is a caller-owned RING of three
 * such planes, batch * per_sample values apart, that holds the last three guided model outputs. With h1 / h2 / h3 the ring planes
 * slot - 1 / slot - 2 / slot - 3 (mod 3) and e the guided (and rescaled) model output as in mi355x_sd_multistep_update, per element:
 *   m   = w0*e [+ w1*h1] [+ w2*h2] [+ w3*h3]       a term whose weight is 0 is not formed and its plane is NOT read
 *   S   = from_park != 0 ? P : x                   from_park: x is NOT read; otherwise P is NOT read
 *   m   = p*S + q*m                                only if p != 0 (v-prediction); p == 0: the product with S is not formed
 *   out = a*S + b*m
 *   plane[slot] <- e                               unless from_park; e as it came from the guidance, before the p / q conversion
 *   P   <- x (bit copy)                            only if park != 0 and from_park == 0
 * Rules:
 *  - coef is 12 fp32 values (a, b, p, q, w0, w1, w2, w3, slot, park, from_park, 0) in device memory, read by the kernel
 *    (PNDMScheduler.plms_coefficients; the twelfth pads the row to 48 bytes and is not read): a captured graph of one node replays a
 *    whole loop, every kind of evaluation, with only the row changing and park / hist at fixed addresses.
 *  - slot is 0, 1 or 2: the number of outputs stored before this one, mod 3. The oldest plane (slot - 3 = slot) is the one e replaces;
 *    each element of it is read (for w3) before it is written, by the same lane, so the ring advances by the row alone and the
 *    launch copies no plane. Any other device value is taken as the nearest of 0, 1, 2 (NaN: 0): nothing outside hist is touched.
 *  - eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 *  - from_park, park, p == 0 and each weight == 0 are wave-uniform branches on the device values. State an evaluation does not need
 *    is not dereferenced: park and hist need no initialising before a loop's first launch (its row has w1 = w2 = w3 = 0 and
 *    from_park = 0), and stale or NaN contents of P, of a ring plane or of x cannot reach out where the row does not use them.
 *  - operation order: as written above, the terms of m summed left to right; which product contracts into which sum is the
 *    compiler's choice, as in mi355x_sd_multistep_update.
 *  - two launches on equal inputs give equal bits (no atomics; the rescale's sums are the fixed trees of mi355x_sd_cfg_rescale_axpby).
 *  - two forms: guidance_rescale > 0 with eps_text runs one 1024-thread block per sample (the statistics passes of
 *    mi355x_sd_cfg_rescale_axpby; a sample of <= 32768 elements stays in registers, larger ones are re-read); otherwise a grid-stride
 *    elementwise kernel with 16-byte vectors when x, park, hist, out and the eps planes are 16-byte aligned and batch * per_sample is
 *    a multiple of 4 (every plane of the ring aligned), and a scalar tail. No scratch memory.
 *  - aliasing: out may be x itself. Any other overlap of out, park or the three planes of hist with each other, x, eps_uncond,
 *    eps_text or coef is MI355X_SD_ERR_INVALID before any launch, as are a null x, eps_uncond, park, hist, out or coef, batch <= 0,
 *    per_sample < 1, and per_sample < 2 with guidance_rescale > 0. */
int mi355x_sd_plms_update(const float* x, const float* eps_uncond, const float* eps_text, float* park, float* hist, float* out,
                          const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                          void* stream);

/* One model evaluation of DPM-Solver singlestep sampling (DPMSolverSinglestepScheduler: dpmsolver++ / dpmsolver, orders 1-3, midpoint /
 * heun) in one launch: guidance combine, guidance rescale, convert_model_output, the update, the parked sample and the group's
 * converted outputs. An order-k evaluation steps from the sample parked k - 1 evaluations earlier, not from the current latents.
 * `park` (S) is one caller-owned plane of batch * per_sample fp32 values; `hist` is two such planes, batch * per_sample values apart:
 * plane 0 holds the first converted output of the current group (an order-1 evaluation and the order-2 and order-3 ones that follow
 * it), plane 1 its second. With e the guided (and rescaled) model output as in mi355x_sd_multistep_update, per element:
 *   m0  = p*x + q*e
 *   order 1:  out = A*x + B*m0                          then S <- x (bit copy), plane 0 <- m0; S and hist are NOT read
 *   order 2:  out = A*S + B*b + E1*(m0 - b)             b = plane 0; plane 1 <- m0 only if keep != 0; S and plane 0 are NOT written
 *   order 3:  out = A*S + B*b + E1*(m0 - b)             b = plane 0
 *                   [+ E2*(m1 - b)]                     m1 = plane 1, only if E2 != 0 (heun); otherwise plane 1 is NOT read
 *                                                       nothing but out is written
 * Rules:
 *  - coef is 8 fp32 values (p, q, A, B, E1, E2, order, keep) in device memory, read by the kernel
 *    (DPMSolverSinglestepScheduler.singlestep_coefficients): a captured graph of one node replays a whole loop, every order, with only
 *    the row changing and park / hist at fixed addresses. keep != 0 on an order-2 row says that an order-3 evaluation follows.
 *  - order is 1, 2 or 3; any other device value is taken as the nearest of them (NaN: 1). An order-k row (k > 1) must directly follow
 *    the order-(k - 1) row of its group: each plane has one writer per group, nothing is shifted and the launch copies no plane.
 *  - eps_text == NULL: no guidance, e = eps_uncond; guidance_scale and guidance_rescale are ignored.
 *  - order, keep and E2 == 0 are wave-uniform branches on the device values. State an evaluation does not need is not dereferenced:
 *    park and hist need no initialising before a loop's first launch (an order-1 row), and stale or NaN contents of S or of a plane
 *    cannot reach out where the row does not use them. x is read by every row.
 *  - operation order: as written above, every difference formed before it is multiplied (E1 and E2 carry the reciprocals of the step
 *    ratios: the regrouped form would cancel), the terms summed left to right; which product contracts into which sum is the
 *    compiler's choice, as in mi355x_sd_multistep_update.
 *  - two launches on equal inputs give equal bits (no atomics; the rescale's sums are the fixed trees of mi355x_sd_cfg_rescale_axpby).
 *  - two forms: guidance_rescale > 0 with eps_text runs one 1024-thread block per sample (the statistics passes of
 *    mi355x_sd_cfg_rescale_axpby; a sample of <= 32768 elements stays in registers, larger ones are re-read); otherwise a grid-stride
 *    elementwise kernel with 16-byte vectors when x, park, hist, out and the eps planes are 16-byte aligned and batch * per_sample is
 *    a multiple of 4 (both planes of hist aligned), and a scalar tail. No scratch memory.
 *  - aliasing: out may be x itself. Any other overlap of out, park or the two planes of hist with each other, x, eps_uncond,
 *    eps_text or coef is MI355X_SD_ERR_INVALID before any launch, as are a null x, eps_uncond, park, hist, out or coef, batch <= 0,
 *    per_sample < 1, and per_sample < 2 with guidance_rescale > 0. */
int mi355x_sd_singlestep_update(const float* x, const float* eps_uncond, const float* eps_text, float* park, float* hist, float* out,
                                const float* coef, float guidance_scale, float guidance_rescale, int batch, int64_t per_sample,
                                void* stream);

/* ---- InstructPix2Pix (StableDiffusionInstructPix2PixPipeline / StableDiffusionXLInstructPix2PixPipeline; ABI 24) ----
 * The three-way guidance combine (pipeline_stable_diffusion_instruct_pix2pix.py:394-400), optionally with rescale_noise_cfg
 * (pipeline_stable_diffusion_xl_instruct_pix2pix.py:105-117, 917-919), into ONE guided plane: what every step-tail entry above takes
 * as its eps_uncond with eps_text == NULL ("already guided"), so the nine tails run behind it with their bits unchanged.
 *   eps     the U-Net output of 3 * batch samples of per_sample floats in the reference's order: t = text, i = image, u = uncond
 *           (plane k starts at eps + k * batch * per_sample)
 *   out     batch samples
 * Per element, IN THIS ORDER (tests/ip2p_bounds.py derives its bound from it; each fma rounds once):
 *   c = fma(guidance_scale, t - i, fma(image_guidance_scale, i - u, u))
 * Three forms:
 *  - guidance_rescale <= 0: out = c. x and coef are ignored (not dereferenced): in real arithmetic the reference's conversion to
 *    predicted originals and back (:388-391, :408-409) cancels, because the weights of t, i, u sum to 1. A grid-stride elementwise
 *    kernel with 16-byte vectors when eps and out are 16-byte aligned and batch * per_sample is a multiple of 4, element by element
 *    otherwise; nothing past the planes is read or written.
 *  - guidance_rescale > 0, x == NULL (a scheduler without `sigmas`): per sample  k = guidance_rescale * std(t) / std(c) + 1 -
 *    guidance_rescale,  out = c * k. std is the unbiased estimator over the sample's per_sample elements, each variance by two passes
 *    (the mean, then the squared deviations), every sum the fixed tree of mi355x_sd_cfg_rescale_axpby: no atomics, equal inputs give
 *    equal bits. One 1024-thread block per sample, no scratch; a sample of <= 32768 elements stays in registers, larger ones are
 *    re-read. A sample of zero variance divides as the reference does (inf / NaN).
 *  - guidance_rescale > 0, x != NULL (a sigma-space scheduler; the reference combines and rescales predicted originals, :903-930):
 *    x is the UNSCALED latents of batch samples, sigma = coef[0] a float in device memory (a row of the loop's sigma table, so a
 *    captured graph replays with another row). p_b = fma(-sigma, e_b, x) for b in t, i, u;  cp = the combine above of p_t, p_i, p_u;
 *    k from std(p_t) and std(cp);  out = (cp * k - x) / (-sigma). sigma == 0 divides by zero: no step of a loop has it.
 * MI355X_SD_ERR_INVALID before any launch: a null eps or out; x without coef (under the rescale); batch <= 0, per_sample < 1,
 * per_sample < 2 with guidance_rescale > 0, 3 * batch * per_sample * 4 bytes past int64_t; out overlapping eps, or -- under the
 * rescale -- x or coef. */
int mi355x_sd_guidance3(const float* eps, const float* x, const float* coef, float* out, float guidance_scale,
                        float image_guidance_scale, float guidance_rescale, int batch, int64_t per_sample, void* stream);
/* The U-Net input of an InstructPix2Pix step in one launch (pipeline_stable_diffusion_instruct_pix2pix.py:373-377:
 * concat([latents] * 3), scheduler.scale_model_input, the channel concat with the image latents). out[g * batch + b], g < groups, is an
 * NCHW sample of c_lat + c_img channels of hw elements:
 *   channels [0, c_lat)              scale * x[b]          one fp32 multiply per element; the same plane for every g
 *   channels [c_lat, c_lat + c_img)  image_latents[g * batch + b]     copied bit for bit
 * x is batch samples of c_lat * hw floats, image_latents groups * batch samples of c_img * hw floats. groups is 3 under guidance and 1
 * without it. 16-byte vectors when the three pointers are 16-byte aligned and c_lat * hw and c_img * hw are multiples of 4, element by
 * element otherwise. MI355X_SD_ERR_INVALID: a null pointer; groups, batch, c_lat, c_img or hw < 1; out's size in bytes past int64_t;
 * out overlapping x or image_latents. MI355X_SD_ERR_UNSUPPORTED: groups * batch > 65535. */
int mi355x_sd_ip2p_input(const float* x, const float* image_latents, float* out, float scale, int groups, int batch, int c_lat,
                         int c_img, int64_t hw, void* stream);

/* ---- Semantic guidance (SEGA: SemanticStableDiffusionPipeline, pipeline_semantic_stable_diffusion.py:541-699; ABI 25) ----
 * ONE launch between the U-Net and a step-tail entry (which takes `out` as its eps_uncond with eps_text == NULL): the classifier-free
 * guidance, every editing concept's quantile-masked direction, the warm-up regimes, the momentum and the caller's extra plane.
 *   eps       the U-Net output of (2 + n_concepts) * batch NCHW samples of channels * hw floats, groups in the reference's order
 *             u = uncond, t = text, e_0 .. e_{n-1}, concept-major (group k starts at eps + k * batch * channels * hw)
 *   momentum  batch samples, read and written in place (zero before the first step; it lives as long as the loop)
 *   extra     the step's sem_guidance plane of batch samples, or NULL
 *   row       this step's row of the table paddlemix_amd/sega_forms.py builds, 8 + 5 * n_concepts 32-bit words in DEVICE memory (a
 *             captured step replays with the next row):
 *               0 regime (int: 0 none warm, 1 partial, 2 all warm)   1 active (int, bit c: concept c is not cooled down)
 *               2 warm (int, bit c)   3 unused   4 gs   5 ms = edit_momentum_scale   6 beta = edit_mom_beta   7 omb = 1 - beta
 *               per concept c at 8 + 5 c:  +0 scale (signed)  +1 lo (int)  +2 frac  +3 w_full  +4 w_part
 *   out       batch samples: the guided noise prediction
 *   stats     NULL, or 3 * n_concepts * batch * channels floats: (v[lo], v[hi], thr) of plane (c, sample, channel), for tests; zeros
 *             for a cooled-down concept
 * Per (sample, channel) plane of hw elements and per active concept c:
 *   g = (e_c - u) * scale                        a subtraction, then a multiplication: the reference's two roundings
 *   v = the ascending order statistics of |g| over the plane; hi = lo when frac == 0, else lo + 1 (lo clamped to [0, hw - 1])
 *   thr = lerp(v[lo], v[hi], frac)               torch.quantile's rule; frac < 0.5: fma(frac, v[hi] - v[lo], v[lo]), otherwise
 *                                                fma(frac - 1, v[hi] - v[lo], v[hi]); NaN when the plane holds a NaN
 *   g_c = |g| >= thr ? g : 0                     (a cooled-down concept: g_c = 0)
 * The selection is EXACT: a radix select over the bit patterns of |g| (they order as unsigned integers) with integer counts in LDS;
 * no floating-point value is reduced across elements, so equal inputs give equal bits. Then per element, IN THIS ORDER
 * (tests/sega_bounds.py derives its bound from it; each fma rounds once):
 *   guid = gs * (t - u)
 *   edit = 0; part = 0;  for c = 0 .. n - 1:  edit = fma(w_full_c, g_c, edit);  if warm bit c:  part = fma(w_part_c, g_c, part)
 *   regime 1:  guid = guid + part
 *   edit = fma(ms, momentum, edit);  momentum' = fma(beta, momentum, omb * edit)
 *   regime 2:  guid = guid + edit
 *   extra:     guid = guid + extra
 *   out = u + guid
 * One block of 1024 threads per (sample, channel); the keys are recomputed from eps on every digit pass (L2-resident), LDS holds a
 * 256-bin histogram. 16-byte loads in the selection when eps is 16-byte aligned and hw % 4 == 0.
 * MI355X_SD_ERR_INVALID before any launch: a null eps, momentum, row or out; n_concepts, batch, channels or hw < 1; a size in bytes
 * past int64_t; momentum, out or stats overlapping any other operand. MI355X_SD_ERR_UNSUPPORTED: n_concepts > 8, hw > 65536 (a
 * 256 x 256 latent), batch * channels > 2^31 - 1. */
int mi355x_sd_sega_guidance(const float* eps, float* momentum, const float* extra, const float* row, float* out, float* stats,
                            int n_concepts, int batch, int channels, int64_t hw, void* stream);

/* ---- Panorama (MultiDiffusion: StableDiffusionPanoramaPipeline, pipeline_stable_diffusion_panorama.py; ABI 26) ----
 * The two passes around the U-Net and the step tails of a panorama step, one launch each. View geometry (the reference's get_views,
 * :473-491, window and stride as arguments): ny x nx views; view v = iy * nx + ix starts at row iy * stride, column ix * stride of the
 * [batch, C, H, W] source and has win_h x win_w elements. Without `circular` every window lies inside the source; with it column j of
 * a view is source column (ix * stride + j) mod W, and rows never wrap.
 *
 * mi355x_sd_view_input: the U-Net input of the views [first, first + count) (:675-709: the slices, the circular concat, the concat
 * over the view batch, the doubling under guidance, scale_model_input). out is [groups][count * batch] NCHW samples of
 * C x win_h x win_w; sample (v - first) * batch + b of EVERY group is scale * x[b] over view v's window: one fp32 multiply per
 * element, the bits of torch's x * scale. groups is 2 under guidance and 1 without it; group-major is this library's
 * [uncond | text] order (what the step tails take as eps and eps + n), not the reference's repeat_interleave. count == 0 launches
 * nothing. 16-byte vectors when W, win_w and stride are multiples of 4 and x and out are 16-byte aligned (a vector then never
 * straddles the wrap); element by element otherwise.
 *
 * mi355x_sd_view_merge: the MultiDiffusion average (:736-754) of all ny * nx views; views is [ny * nx * batch] samples, view v of
 * image b at v * batch + b. Every element of out [batch, C, H, W] is written exactly once, in GATHER form: the views that cover it are
 * visited in ascending v, their values added one by one in fp32 to a sum that starts at +0.0f, the sum divided by their number with
 * a correctly rounded fp32 division -- the reference's value / count / where(count > 0, value / count, value) bit for bit: no
 * atomics, no reciprocal, no reassociation. An element no view covers (without `circular`, the columns past the last window when
 * (W - win_w) % stride != 0) gets the sum itself, +0.0f. The same vector rule, with views in place of x.
 *
 * MI355X_SD_ERR_INVALID before any launch, the message naming the argument: a null pointer; groups not 1 or 2; batch, C, H, W, win_h,
 * win_w, stride, ny or nx < 1; win_h > H or win_w > W; (ny - 1) * stride + win_h > H; without `circular` (nx - 1) * stride + win_w > W,
 * with it (nx - 1) * stride >= W; first or count outside [0, ny * nx] or first + count > ny * nx; a size in bytes past int64_t; out
 * overlapping x / views. MI355X_SD_ERR_UNSUPPORTED: count * batch * C (view_input) or batch * C (view_merge) > 65535, or more than
 * 4 * 65535 rows in a window (view_input) or in the source (view_merge). */
int mi355x_sd_view_input(const float* x, float* out, float scale, int groups, int batch, int C, int H, int W, int win_h, int win_w,
                         int stride, int ny, int nx, int circular, int first, int count, void* stream);
int mi355x_sd_view_merge(const float* views, float* out, int batch, int C, int H, int W, int win_h, int win_w, int stride, int ny,
                         int nx, int circular, void* stream);

/* hipGraph capture of a sequence of the calls above issued on `stream` (one denoising step). */
int mi355x_sd_graph_begin(void* stream);
int mi355x_sd_graph_end(void* stream, void** graph_exec);
int mi355x_sd_graph_launch(void* graph_exec, void* stream);
int mi355x_sd_graph_destroy(void* graph_exec);

/* ---- multi-GPU (paddlemix_amd/csrc/comm.hip): what a plain-C host needs for "a batch of independent prompts shards across the
 * GPUs of a node with an RCCL broadcast of the text-encoder / UNet weights over xGMI" (SURVEY.md 8e). One process per GPU. Rank 0 packs
 * the weights (mi355x_sd_unet_finalize_weights / mi355x_sd_program_bind write them into ONE caller-owned device buffer), every rank
 * allocates a buffer of the same size and receives it in place with mi355x_sd_comm_broadcast; each rank then denoises its own prompts
 * with no per-step collective (batch rows never interact), and mi355x_sd_comm_all_gather collects the ranks' latents once at the end.
 * The reference's precedent: the batch-parallel mode of its SD3 pipeline (PPD/pipelines/stable_diffusion_3/
 * pipeline_stable_diffusion_3.py:803-839). `id128`: 128 opaque bytes made by rank 0 (mi355x_sd_comm_unique_id) and carried to the
 * other ranks by the host's own means (file, socket, launcher environment). Collectives are stream-ordered on `stream`; byte counts,
 * no element type. RCCL is loaded with dlopen at the first call: a machine without it still loads the library, these five entry
 * points then return MI355X_SD_ERR_UNSUPPORTED with the reason in mi355x_sd_last_error(). */
int mi355x_sd_comm_unique_id(void* id128);
int mi355x_sd_comm_init(const void* id128, int rank, int world, void** comm);
int mi355x_sd_comm_broadcast(void* comm, void* buf, size_t bytes, int root, void* stream);
int mi355x_sd_comm_all_gather(void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream);
int mi355x_sd_comm_destroy(void* comm);

/* Test hook: dumps the lane->element maps of the MFMA / LDS-transpose instructions the kernels rely on
 * (out: 64*(4+16+4) floats, see tests/test_gpu_probe.py). */
int mi355x_sd_probe_layouts(float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
