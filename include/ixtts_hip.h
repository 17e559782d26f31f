/* ixtts_hip.h -- C ABI of libixtts_hip.so: the MI355X (gfx950) hot path of IndexTTS2.
 *
 * Drop-in boundary for ONE path of caishiqing/voice-tts: the autoregressive GPT decode
 * step and the BigVGAN vocoder of `indextts.infer_v2.IndexTTS2.infer()`.
 * Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * Conventions
 *   - every `*_dev` pointer is DEVICE memory on the current HIP device; `*_host` is host memory;
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream); all
 *     compute entry points are asynchronous on it unless stated otherwise;
 *   - return value: 0 on success, a negative IXTTS_ERR_* code otherwise; no C++
 *     exception crosses the ABI; `ixtts_last_error()` gives the text of the last failure
 *     on the calling thread;
 *   - handles are not re-entrant: one in-flight call per handle (the reference serialises
 *     `infer()` behind `inference_lock`, server.py:25,384).
 *
 * Each entry point cites the reference interface it replaces (paths relative to the
 * reference repo root).
 */
#ifndef IXTTS_HIP_H
#define IXTTS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IXTTS_OK 0
#define IXTTS_ERR_ARG (-1)   /* bad argument / shape mismatch          */
#define IXTTS_ERR_HIP (-2)   /* a HIP runtime call failed               */
#define IXTTS_ERR_STATE (-3) /* call order violated (e.g. not finalized) */
#define IXTTS_ERR_NOMEM (-4) /* device/host allocation failed           */
#define IXTTS_ERR_NAME (-5)  /* unknown tensor name                     */

const char* ixtts_version(void);
const char* ixtts_last_error(void);

/* ------------------------------------------------------------------------------------
 * Seam 3 -- fused anti-aliased SnakeBeta activation
 * replaces: `extern "C" torch::Tensor fwd_cuda(input, up_filter, down_filter, alpha, beta)`
 *   indextts/s2mel/modules/bigvgan/alias_free_activation/cuda/anti_alias_activation.cpp:19-22
 *   indextts/s2mel/modules/bigvgan/alias_free_activation/cuda/anti_alias_activation_cuda.cu:212-246
 * y[b,c,:] = Down2(SnakeBeta(Up2(x[b,c,:]))), 12-tap filters, replicate padding, log-scale
 * alpha/beta [C] (exp applied inside, .cu:86-89).  Semantics follow the reference's CPU
 * (torch) path `alias_free_activation/torch/act.py:24-30` exactly, including the sequence
 * edges.  x, y: [B,C,T] contiguous fp32; y may not alias x.  T == 0 is a no-op.
 */
int ixtts_aa_snake_f32(const float* x_dev, float* y_dev, const float* up12_dev, const float* down12_dev,
                       const float* log_alpha_dev, const float* log_beta_dev, int B, int C, int T, void* stream);

/* ------------------------------------------------------------------------------------
 * Row N1 helper -- full (unmasked, non-causal) fp32 attention of the s2mel DiT
 * replaces: `F.scaled_dot_product_attention(q, k, v, attn_mask=mask)` with an all-true mask
 *   indextts/s2mel/modules/gpt_fast/model.py:303 (called from diffusion_transformer.py:238)
 * q, k, v, out: fp32, element (b, t, h, d) at base[b*stride_b + t*stride_t + h*stride_h + d] (d contiguous,
 * head_dim 64, strides in floats and multiples of 4); out = softmax(scale * q k^T) v per (b, h).
 * workspace_dev (optional, ixtts_attn_full_workspace_bytes(B,H,T) bytes of scratch owned by the caller): holds the K / V operand
 * planes of the default kernel (csrc/attn_full_x3.hip: every fp32 product as six bf16 MFMA partial products of exactly split
 * operands, fp32 accumulate -- fp32-quality results, tests/test_gpu_s2mel.py) and the partials of the key-range split it uses when
 * the un-split grid cannot fill the GPU (+ a merge pass).  Without it, or with IXTTS_ATTN_FULL=f32 in the environment, the
 * fp32-MFMA kernel of csrc/attn_full.hip runs.
 */
size_t ixtts_attn_full_workspace_bytes(int B, int H, int T);
int ixtts_attn_full_f32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, int B, int H, int T,
                        int head_dim, long stride_b, long stride_t, long stride_h, long ostride_b, long ostride_t,
                        long ostride_h, float scale, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ixtts_attn_full_varlen_f32: the same attention (x3 arithmetic) over n PACKED sequences of unequal length: sequence s owns rows
 * [seq_off[s], seq_off[s+1]) of q, k, v, out (element (row, h, d) at base[row*stride_t + h*stride_h + d]), and its queries see its
 * own keys only.  table_dev (int32, device) = [seq_off (nseq + 1) | tile_off (nseq + 1) | n_work (sequence, 128-query block) pairs]:
 * tile_off the prefix sums of ceil(T_s / 64) (total_tiles = tile_off[nseq]), every (s, block) with block < ceil(T_s / 128) listed
 * once, every T_s >= 1.  workspace_dev: ixtts_attn_full_varlen_workspace_bytes(nseq, H, total_tiles) bytes (the K / V planes; the
 * key range is never split).  IXTTS_ATTN_FULL is not read: callers wanting the fp32-MFMA kernel call the entry above per sequence.
 */
size_t ixtts_attn_full_varlen_workspace_bytes(int nseq, int H, int total_tiles);
int ixtts_attn_full_varlen_f32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, const int* table_dev, int nseq,
                               int total_tiles, int n_work, int H, int head_dim, long stride_t, long stride_h, long ostride_t, long ostride_h,
                               float scale, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ixtts_attn_full_rope_f32 / ixtts_attn_full_rope_varlen_f32: the two entries above with RoPE (gpt_fast/model.py:289-301,348-360) of
 * q and k inside: q and k arrive UNROTATED (and are left so), the keys are rotated as they are split into planes, the queries as they
 * are loaded, v is untouched.  cos_sin_dev [positions][32] (cos, sin) pairs, 16-byte aligned, position = row within the sequence
 * (rope_rows >= T; varlen: it covers the longest sequence).  Bit for bit ixtts_rope_qk_f32 (/ _varlen_f32) on q and k followed by
 * the entry above.  Split-product build only: workspace_dev is required, and IXTTS_ATTN_FULL=f32 is refused. */
int ixtts_attn_full_rope_f32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, const float* cos_sin_dev, int rope_rows,
                             int B, int H, int T, int head_dim, long stride_b, long stride_t, long stride_h, long ostride_b, long ostride_t,
                             long ostride_h, float scale, void* workspace_dev, size_t workspace_bytes, void* stream);
int ixtts_attn_full_rope_varlen_f32(const float* q_dev, const float* k_dev, const float* v_dev, float* out_dev, const float* cos_sin_dev,
                                    const int* table_dev, int nseq, int total_tiles, int n_work, int H, int head_dim, long stride_t, long stride_h,
                                    long ostride_t, long ostride_h, float scale, void* workspace_dev, size_t workspace_bytes, void* stream);

/* Row N1 helpers -- the element/row chains between the DiT's GEMMs, one fp32 pass each (csrc/dit_ops.hip).
 *
 * ixtts_adaln_rmsnorm_f32  replaces AdaptiveLayerNorm.forward over RMSNorm (gpt_fast/model.py:18-37,362-372):
 *     out[b,t,:] = wb[b,H:2H] + wb[b,0:H] * (x[b,t,:] * rsqrt(mean(x^2) + eps) * g), wb = project_layer(c) [B,2H].
 * ixtts_ln_modulate_f32    replaces FinalLayer's `modulate(norm_final(x), shift, scale)` (diffusion_transformer.py:83-100):
 *     out = layer_norm(x, eps, no affine) * (1 + ss[b,H:2H]) + ss[b,0:H], ss = adaLN_modulation(c) [B,2H] (shift | scale).
 * ixtts_rope_qk_f32        replaces apply_rotary_emb on q and k (gpt_fast/model.py:289-301,348-360), in place on the
 *     wqkv output [B*T,3H]: pair i of head h at columns h*hd+2i,+1 is multiplied by cos_sin[t][i] = (cos, sin).
 * ixtts_swiglu_f32         replaces `F.silu(w1(x)) * w3(x)` (gpt_fast/model.py:316-326) on the fused [w1; w3] GEMM
 *     output u [rows,2F]: out[r,j] = silu(u[r,j]) * u[r,F+j].
 * ixtts_wn_gate_f32        replaces fused_add_tanh_sigmoid_multiply (wavenet.py:142-160): out[b,c,t] =
 *     tanh(a[b,c,t] + g[b,off+c]) * sigmoid(a[b,C+c,t] + g[b,off+C+c]); a [B,2C,T], g [B,g_stride], out [B,C,T].
 * ixtts_wn_gate_rows_f32   the same gate in row layout: a [rows,2C] -> out [rows,C], row r taking the gate biases of batch
 *     entry min(r / rows_per_batch, B-1) (the WaveNet head keeps its sequences as rows so that every conv is a plain
 *     row-major GEMM; rows between two sequences are computed and never read).
 * ixtts_reflect_halo_rows_f32  refreshes the reflect padding (SConv1d pad_mode "reflect", wavenet.py:103-140) of a row-layout
 *     buffer p [B, left+T+right, C] in place from its interior rows.
 * All tensors contiguous fp32 device memory; H, F, C multiples of 4, H <= 2048.
 */
int ixtts_adaln_rmsnorm_f32(const float* x_dev, const float* wb_dev, const float* g_dev, float* out_dev, int B, int T, int H, float eps,
                            void* stream);
int ixtts_ln_modulate_f32(const float* x_dev, const float* shift_scale_dev, float* out_dev, int B, int T, int H, float eps, void* stream);
int ixtts_rope_qk_f32(float* qkv_dev, const float* cos_sin_dev, int B, int T, int H, int head_dim, void* stream);
int ixtts_swiglu_f32(const float* u_dev, float* out_dev, long rows, int F, void* stream);
int ixtts_wn_gate_f32(const float* a_dev, const float* g_dev, float* out_dev, int B, int C, int T, long g_stride, int g_offset, void* stream);
int ixtts_wn_gate_rows_f32(const float* a_dev, const float* g_dev, float* out_dev, long rows, int C, long rows_per_batch, int B, long g_stride,
                           int g_offset, void* stream);
int ixtts_reflect_halo_rows_f32(float* p_dev, int B, int T, int C, int left, int right, void* stream);

/* The same row ops over n PACKED sequences of unequal length: seq_off_dev (int32, device) [nseq + 1] ascending row offsets, sequence s
 * owning rows [seq_off[s], seq_off[s+1]), rows = seq_off[nseq] (the gate: rows past seq_off[nseq] take the last sequence's biases).
 * ixtts_adaln_rmsnorm_varlen_f32 / ixtts_ln_modulate_varlen_f32: row r takes row s of wb / shift_scale [nseq, 2H].
 * ixtts_rope_qk_varlen_f32: positions restart at 0 in each sequence (cos_sin covers the longest one).
 * ixtts_wn_gate_rows_varlen_f32: row r takes the gate biases g[s * g_stride + g_offset ...] of its sequence.
 * ixtts_reflect_halo_rows_varlen_f32: sequence s = left halo | T_s interior | right halo rows, T_s > max(left, right) (a shorter
 *     sequence is left untouched; the caller refuses it).
 */
int ixtts_adaln_rmsnorm_varlen_f32(const float* x_dev, const float* wb_dev, const float* g_dev, float* out_dev, const int* seq_off_dev, int nseq,
                                   long rows, int H, float eps, void* stream);
int ixtts_ln_modulate_varlen_f32(const float* x_dev, const float* shift_scale_dev, float* out_dev, const int* seq_off_dev, int nseq, long rows, int H,
                                 float eps, void* stream);
int ixtts_rope_qk_varlen_f32(float* qkv_dev, const float* cos_sin_dev, const int* seq_off_dev, int nseq, long rows, int H, int head_dim, void* stream);
int ixtts_wn_gate_rows_varlen_f32(const float* a_dev, const float* g_dev, float* out_dev, long rows, int C, const int* seq_off_dev, int nseq,
                                  long g_stride, int g_offset, void* stream);
int ixtts_reflect_halo_rows_varlen_f32(float* p_dev, const int* seq_off_dev, int nseq, int C, int left, int right, void* stream);

/* AdaLN-RMSNorm whose output goes straight to a split-product GEMM: the same rows as ixtts_adaln_rmsnorm_f32 (/ _varlen_f32), written
 * as the bf16 planes that ixtts_gemm_x6_split would make of them -- byte for byte, the zero rows up to ixtts_gemm_x6_rows_padded(rows)
 * included -- instead of as fp32 (which is not written).  planes_dev: (H/16) * 6 * rows_padded * 16 bytes, 128-byte aligned; H a
 * multiple of 64, at most 1024. */
int ixtts_adaln_rmsnorm_planes_f32(const float* x_dev, const float* wb_dev, const float* g_dev, void* planes_dev, int B, int T, int H, float eps,
                                   void* stream);
int ixtts_adaln_rmsnorm_planes_varlen_f32(const float* x_dev, const float* wb_dev, const float* g_dev, void* planes_dev, const int* seq_off_dev,
                                          int nseq, long rows, int H, float eps, void* stream);

/* Row N1 -- the linear layers of the s2mel DiT / WaveNet: C[M][N] (+)= A[M][K] . W[N][K]^T + bias, fp32 in and out
 * replaces: `nn.Linear` / 1x1 and k-tap Conv1d of indextts/s2mel/modules/gpt_fast/model.py:242-326 (wqkv, wo, w1 | w3, w2),
 *   wavenet.py:103-174 (in_layers as one row-shifted GEMM per tap, res_skip_layers), diffusion_transformer.py:186-257 (merge / skip
 *   linears), called through torch's fp32 library GEMMs in r02.
 * Arithmetic (csrc/gemm_x6.hip): every fp32 product as six exact bf16 MFMA partial products of three-way split operands, fp32
 * accumulation -- fp32-quality results (tests/test_gpu_gemm_x6.py: error against fp64 no larger than the fp32 library GEMM's).
 * Operands travel as bf16 PLANES [K/16][plane 3][k-half 2][rows_padded] of 16-byte units (eight consecutive k of one row):
 *   ixtts_gemm_x6_pack   splits a weight matrix W [N][K] (fp32, row-major, K a multiple of 64) once, at load, into
 *                        ixtts_gemm_x6_packed_bytes(N, K) bytes of device memory owned by the caller;
 *   ixtts_gemm_x6_split  splits activations A [rows][K] (row stride lda floats, 16-byte aligned rows) into planes of
 *                        ixtts_gemm_x6_rows_padded(rows) rows: (K/16) * 6 * rows_padded * 16 bytes owned by the caller;
 *   ixtts_gemm_x6_f32    C[M][N] (row stride ldc) (+)= A[row0 .. row0 + M) . W^T + bias over planes holding rows_total rows (a
 *                        row-shifted window of one split buffer = one tap of a k-tap Conv1d); bias_dev [N] or NULL; accumulate != 0
 *                        adds to what C holds (torch's addmm_); tile: 0 = chosen by the fill of the 256 CUs, 2 / 3 = 256x128 /
 *                        128x128, 6 = 128x128 on the pipelined loop, one workgroup per CU (what 0 picks in place of 3 when
 *                        there are no more 128x128 tiles than CUs; IXTTS_GEMM_X6_PIPE=0 keeps 3) -- the same bytes from
 *                        every tile (A/B timing). */
size_t ixtts_gemm_x6_packed_bytes(int N, int K);
int ixtts_gemm_x6_pack(const float* w_dev, void* packed_dev, int N, int K, void* stream);
long ixtts_gemm_x6_rows_padded(long rows);
int ixtts_gemm_x6_split(const float* a_dev, long lda, void* planes_dev, long rows, int K, void* stream);
int ixtts_gemm_x6_f32(const void* a_planes_dev, long rows_total, long row0, const void* packed_dev, const float* bias_dev, float* c_dev, long ldc,
                      int M, int N, int K, int accumulate, int tile, void* stream);
/* ixtts_gemm_x6_split_halo (/ _varlen): ixtts_gemm_x6_split of a reflect-padded row buffer (rows = whole sequences of left + T + right
 * rows; varlen: sequence s = rows [seq_off[s], seq_off[s+1]), its own halo rows included, rows = seq_off[nseq]) that reads every halo
 * row from the interior row it mirrors: the planes of ixtts_reflect_halo_rows_f32 (/ _varlen_f32) followed by ixtts_gemm_x6_split,
 * without the refresh -- the fp32 halo rows are neither read nor written. */
int ixtts_gemm_x6_split_halo(const float* a_dev, long lda, void* planes_dev, long rows, int K, int T, int left, int right, void* stream);
int ixtts_gemm_x6_split_halo_varlen(const float* a_dev, long lda, void* planes_dev, long rows, int K, const int* seq_off_dev, int nseq, int left,
                                    int right, void* stream);
/* ixtts_gemm_x6_pair_f32: the same GEMM with a pair epilogue, over weights packed with their two halves interleaved in 32-row blocks
 * (rows 64q .. 64q + 31 = rows 32q .. of the first half, 64q + 32 .. 64q + 63 = the same rows of the second; bias_dev [N] likewise):
 * C[M][N/2] = f(a, b), a / b = the two halves' results + bias; epilogue 1 = silu(a) * b (SwiGLU), 2 = tanh(a + g_a) * sigmoid(b + g_b)
 * with (g_a | g_b) = gate_dev[min(r / rows_per_batch, nbatch - 1) * gate_ld + (0 .. N)) for output row r (the WaveNet gate).  taps > 1:
 * K = taps x K_a over planes of K_a columns, k block j of the weights reading the planes' rows shifted down by j (a k-tap Conv1d over a
 * row buffer in one GEMM; rows row0 .. row0 + M + taps - 1 of rows_total are read).  N a multiple of 64; tile 0 / 2 / 3 / 6 as above. */
int ixtts_gemm_x6_pair_f32(const void* a_planes_dev, long rows_total, long row0, int taps, const void* packed_dev, const float* bias_dev,
                           const float* gate_dev, long gate_ld, long rows_per_batch, int nbatch, float* c_dev, long ldc, int M, int N, int K,
                           int epilogue, int tile, void* stream);
/* ixtts_gemm_x6_pair_gate_varlen_f32: the gate epilogue (2) over a row buffer of n packed sequences: output row r takes the gate biases
 * gate_dev[s * gate_ld + ...] of the s with seq_off[s] <= r < seq_off[s+1] (seq_off_dev: int32 device table [nseq + 1], the padded
 * offsets -- each sequence with its own halo rows; rows past seq_off[nseq] take the last sequence's). */
int ixtts_gemm_x6_pair_gate_varlen_f32(const void* a_planes_dev, long rows_total, long row0, int taps, const void* packed_dev, const float* bias_dev,
                                       const float* gate_dev, long gate_ld, const int* seq_off_dev, int nseq, float* c_dev, long ldc, int M, int N,
                                       int K, int tile, void* stream);

/* ------------------------------------------------------------------------------------
 * Seam 2 -- BigVGAN-v2 generator
 * replaces: `BigVGAN.__init__/remove_weight_norm/forward`
 *   indextts/s2mel/modules/bigvgan/bigvgan.py:266-400 ; call site indextts/infer_v2.py:154-158,735
 */
#define IXTTS_BIGVGAN_MAX_STAGES 8
#define IXTTS_BIGVGAN_MAX_RESK 4

typedef struct ixtts_bigvgan_cfg {
  int num_mels;                 /* 80   (config.json:44) */
  int upsample_initial_channel; /* 1536 (config.json:13) */
  int n_stages;                 /* 6 */
  int upsample_rates[IXTTS_BIGVGAN_MAX_STAGES];        /* 4,4,2,2,2,2 */
  int upsample_kernel_sizes[IXTTS_BIGVGAN_MAX_STAGES]; /* 8,8,4,4,4,4 */
  int n_resblock_kernels;       /* 3 */
  int resblock_kernel_sizes[IXTTS_BIGVGAN_MAX_RESK];   /* 3,7,11 */
  int resblock_dilations[IXTTS_BIGVGAN_MAX_RESK][3];   /* 1,3,5 each */
  int max_frames;               /* workspace is sized for mel lengths up to this */
  int fast_sin;                 /* 0: libm-accurate sinf in the Snake (parity mode); 1: v_sin_f32 */
} ixtts_bigvgan_cfg;

typedef struct ixtts_bigvgan ixtts_bigvgan;

int ixtts_bigvgan_create(ixtts_bigvgan** out, const ixtts_bigvgan_cfg* cfg);
/* Upload one tensor of the weight-norm-FOLDED generator state dict by its reference name
 * ("conv_pre.weight", "ups.0.0.weight", "resblocks.3.convs1.2.bias",
 *  "resblocks.3.activations.5.act.alpha", "activation_post.act.beta", "conv_post.weight"...).
 * `data_host` is fp32 in the reference's own layout; the library re-packs it. */
int ixtts_bigvgan_set_tensor(ixtts_bigvgan* h, const char* name, const float* data_host, const int64_t* shape, int ndim);
/* Verifies every tensor was supplied. */
int ixtts_bigvgan_finalize(ixtts_bigvgan* h);
/* Packed weight arena (device), for a one-shot RCCL broadcast at load: after
 * `finalize` on rank 0 and `adopt_arena` elsewhere the handles are equivalent. */
int ixtts_bigvgan_arena(ixtts_bigvgan* h, void** ptr_dev, size_t* bytes);
int ixtts_bigvgan_adopt_arena(ixtts_bigvgan* h);
/* mel [B,num_mels,F] fp32 -> wav [B,1,F*prod(rates)] fp32, clamp(-1,1) (bigvgan.py:360-386). */
int ixtts_bigvgan_forward(ixtts_bigvgan* h, const float* mel_dev, int B, int F, float* wav_dev, void* stream);
/* The same generator over B rows of unequal length in one pass: mel [B,num_mels,Fmax] and wav [B,1,Fmax*prod(rates)] are padded to
 * Fmax, row b is frames[b] frames long.  `frames_dev` is what the kernels read (each clamps it to [0, Fmax], so no table can move
 * a load or a store outside the tensors); `frames_host` holds the same numbers for validation (0 <= frames <= Fmax, else
 * IXTTS_ERR_ARG) and for choosing conv tiles.  Padding is never read -- it may hold anything, NaN included -- and wav_dev[b] from
 * frames[b]*prod(rates) on is left untouched; a row of 0 frames writes nothing; B == 0 or Fmax == 0 returns IXTTS_OK.  Row b is
 * bit-identical to ixtts_bigvgan_forward on that row alone.  Same schedule and workspace (sized for B x Fmax). */
int ixtts_bigvgan_forward_varlen(ixtts_bigvgan* h, const float* mel_dev, const int* frames_dev, const int* frames_host, int B, int Fmax,
                                 float* wav_dev, void* stream);
/* Conv launches of this handle so far, by tile shape (rows x columns): plain host counters, incremented where the launcher
 * decides; no device work.  `*f32_convs` tells which kernels the handle runs and so what the six slots are:
 *   0 (default, conv1d_x3.hip):        128x128, 128x96, 64x128 chosen by score | 32x128, 64x128 fixed by Cout | unused
 *   1 (IXTTS_BV_CONV=f32, conv1d.hip): 128x128, 64x128, 64x64  chosen by score | 32x256, 64x128, 96x128 fixed by Cout
 * The developer switch IXTTS_BV_TILE=<one of the three scored names of the handle's kernels>, read by ixtts_bigvgan_create,
 * puts that tile wherever the launcher would choose by score (convs on a fixed tile ignore it); any other value makes create
 * fail with IXTTS_ERR_ARG. */
#define IXTTS_BIGVGAN_TILE_SLOTS 6
int ixtts_bigvgan_tile_launches(const ixtts_bigvgan* h, int64_t* counts /* [IXTTS_BIGVGAN_TILE_SLOTS] */, int* f32_convs);
/* Algorithmic conv FLOPs of one forward at F frames. */
double ixtts_bigvgan_flops(const ixtts_bigvgan* h, int B, int F);
int ixtts_bigvgan_destroy(ixtts_bigvgan* h);

/* ------------------------------------------------------------------------------------
 * Seam 1 -- autoregressive GPT-2 decode engine
 * replaces: the object DeepSpeed swaps in for `UnifiedVoice.inference_model`
 *   indextts/gpt/model_v2.py:433-446 (seam), :45-212 (GPT2InferenceModel),
 *   :663-734 (inference_speech -> store_mel_emb + generate), :554-596 (latent forward);
 *   trunk arithmetic indextts/gpt/transformers_gpt2.py:480-667,985-1184;
 *   token selection indextts/gpt/transformers_generation_utils.py:843-1070,3123-3297.
 */
#define IXTTS_DTYPE_F32 0
#define IXTTS_DTYPE_BF16 1
#define IXTTS_DTYPE_F16 2
/* weight_dtype of the GPT: the type of the five matrices per layer + mel_head in the arena AND of the K/V cache (vectors,
 * embeddings, the residual stream and every accumulation stay fp32).
 *   F32   parity mode: bit-exact against the fp32 oracle.
 *   BF16  throughput mode (what `use_fp16=True` selects by default).
 *   F16   IEEE half, the precision the reference serves with `use_fp16=True`: same bytes per step as BF16, three more
 *         mantissa bits.  Weights are rounded to nearest even at finalize; a folded weight beyond +-65504 is never stored
 *         as inf -- ixtts_gpt_finalize returns IXTTS_ERR_ARG ("fp16 overflow") instead.  Every fp32 -> fp16 conversion of an
 *         activation or a K/V row saturates at +-65504 (no inf, no NaN).  IXTTS_WIDE=1 applies as it does to BF16;
 *         IXTTS_MLP=fused is a BF16 kernel and is ignored.
 * ixtts_gpt_share_arena refuses two engines of different weight_dtype. */

typedef struct ixtts_gpt_cfg {
  int model_dim;       /* 1280 */
  int layers;          /* 24   */
  int heads;           /* 20   (head dim must be 64) */
  int n_mel_codes;     /* 8194 (vocabulary of mel_head / mel_embedding) */
  int n_mel_pos;       /* rows of mel_pos_embedding (max_mel_tokens + 3 = 1818) */
  int n_text_tokens;   /* rows of text_embedding (12001) */
  int n_text_pos;      /* rows of text_pos_embedding (602) */
  int start_mel_token; /* 8192 */
  int stop_mel_token;  /* 8193 */
  int max_seq;         /* KV-cache capacity per sequence (prompt + generated) */
  int max_batch;       /* concurrent sequences: 1..ixtts_gpt_max_batch_for(weight_dtype) (32 for bf16 / f16, 16 for f32) */
  int weight_dtype;    /* IXTTS_DTYPE_F32 (parity mode) | IXTTS_DTYPE_BF16 (throughput mode) | IXTTS_DTYPE_F16 (see above) */
} ixtts_gpt_cfg;

#define IXTTS_NGRAM_MAX 8     /* largest no_repeat_ngram_size */
#define IXTTS_SEQ_BIAS_MAX 64 /* entries of a sequence's bias table: `sequence_bias` and `bad_words_ids` share it */
#define IXTTS_SEQ_BIAS_LEN 8  /* ids per entry */

/* Token selection follows `_get_logits_processor` (transformers_generation_utils.py:862-1069), in its order:
 *   [suppress_stop] -> SequenceBias -> RepetitionPenalty -> NoRepeatNGram -> NoBadWords -> MinNewTokens -> ForcedEOS
 *   -> ExponentialDecayLengthPenalty -> SuppressTokens -> SuppressTokensAtBegin -> [typical]
 *   -> Temperature -> TopK -> TopP -> MinP -> EpsilonCutoff -> EtaCutoff -> LogitNormalization -> softmax + multinomial | argmax
 * The warpers (Temperature .. EtaCutoff) run when sampling only: not in greedy decoding, not in beam search proper. */
typedef struct ixtts_sampler_cfg {
  float repetition_penalty; /* 10.0 (infer_v2.py:605); 1.0 disables                         */
  float temperature;        /* 0.8; ignored when do_sample == 0                              */
  int top_k;                /* 30; 0 (or >= vocabulary) disables the filter; any value for sampling, 1..128 in beam mode;
                               "greedy" of BASELINE configs == do_sample 0 or top_k 1 */
  float top_p;              /* 0.8                                                           */
  int do_sample;            /* 0: argmax of penalised logits; 1: multinomial after warpers.  Beam mode: 1 = beam-sample (the served
                               default), 0 = beam search proper -- the joint top 2 * num_beams, the warpers do not run
                               (transformers_generation_utils.py:1020,3520-3524) */
  int suppress_stop;        /* bench-only fixed-length mode: stop token forced to -inf       */
  uint64_t seed;            /* Philox seed for do_sample (cannot match torch's CPU stream)   */
  float typical_mass;       /* > 0: the custom TypicalLogitsWarper of `inference_speech(typical_sampling=True, typical_mass=...)`
                               (model_v2.py:717-722, utils/typical_sampling.py) after the repetition penalty; 0: off */
  float length_penalty;     /* beam mode: hypothesis score = sum_logprobs / generated_len ** length_penalty
                               (transformers_beam_search.py:947-951,989-1006); 0.0 is the served default (infer_v2.py:603) */
  /* The constraints `generate()` builds from plain keywords (transformers_generation_utils.py:902-1049); 0 = off.  Like every field
     they belong to the slot / the beam group.  The two id lists of the family are state of the sequence: ixtts_gpt_set_bans. */
  int min_new_tokens;       /* MinNewTokensLengthLogitsProcessor: the stop token is -inf while fewer tokens than this have been
                               generated; more than can be generated is no error (the sequence runs to its cap); >= 0 */
  int no_repeat_ngram_size; /* NoRepeatNGramLogitsProcessor over the history HF sees -- the fake prompt ids [1]*(P-1) + [start_mel]
                               and the generated tokens (in beam mode each beam's own reordered history): the token that followed an
                               earlier occurrence of the last n-1 tokens is -inf; 1 bans every id of the history;
                               0..IXTTS_NGRAM_MAX */
  float min_p;              /* MinPLogitsWarper, sampling (and beam-sample) only, after TopP: ids whose probability over the remaining
                               scores is below min_p * the largest are removed, the best min_tokens_to_keep (1; 2 with beams)
                               never; 0..1 */
  /* The rest of that family (transformers_generation_utils.py:862-1069); 0 = off, so a caller that zero-fills them gets none of it.
     The table of biased sequences and the forced ids are state of the sequence: ixtts_gpt_set_sequence_bias, ixtts_gpt_set_forced_eos. */
  int exp_decay_start;      /* ExponentialDecayLengthPenalty(start_index, factor): once MORE than exp_decay_start tokens have been */
  double exp_decay_factor;  /* generated, score[stop] += |score[stop]| * (factor ** (generated - start) - 1); the power is taken in fp64
                               as HF takes it in Python floats, so the factor is a double; a stop score of -inf stays -inf.
                               factor 0: off; start >= 0, factor > 0 */
  float epsilon_cutoff;     /* EpsilonLogitsWarper, sampling only, after MinP: ids whose probability over the remaining scores is
                               below epsilon are removed, the best min_tokens_to_keep (1; 2 with beams) never; [0, 1) */
  float eta_cutoff;         /* EtaLogitsWarper, after it: the same with the threshold min(eta, sqrt(eta) * exp(-entropy)); [0, 1) */
  int renormalize_logits;   /* LogitNormalization, last: the scores become their own log_softmax.  Without beams that changes neither
                               tokens nor ixtts_gpt_read_probs; with beams each beam's candidate scores are shifted by the logsumexp
                               over that beam's surviving scores (beam search proper: over its whole processed row) */
  int forced_eos_step;      /* ForcedEOSTokenLogitsProcessor: when the forced_eos_step-th generated token is chosen (HF: the token at
                               position max_length - 1, so forced_eos_step = max_length - prompt length) every score is -inf and the
                               ids of ixtts_gpt_set_forced_eos are 0; SuppressTokens still runs after it.  >= 0 */
  int n_seq_bias;           /* filled in by the engine (entries of the slot's / the group's table); whatever the caller writes here
                               is ignored */
} ixtts_sampler_cfg;

typedef struct ixtts_gpt ixtts_gpt;

int ixtts_gpt_create(ixtts_gpt** out, const ixtts_gpt_cfg* cfg);
/* Upload one tensor of `UnifiedVoice.state_dict()` by name, fp32 host data in the
 * reference layout: gpt.h.{i}.{ln_1,ln_2}.{weight,bias}, gpt.h.{i}.attn.{c_attn,c_proj}.{weight,bias},
 * gpt.h.{i}.mlp.{c_fc,c_proj}.{weight,bias}, gpt.ln_f.*, final_norm.*, mel_head.*,
 * mel_embedding.weight, mel_pos_embedding.emb.weight.  Other names return IXTTS_ERR_NAME. */
int ixtts_gpt_set_tensor(ixtts_gpt* h, const char* name, const float* data_host, const int64_t* shape, int ndim);
int ixtts_gpt_finalize(ixtts_gpt* h);
int ixtts_gpt_arena(ixtts_gpt* h, void** ptr_dev, size_t* bytes);
int ixtts_gpt_adopt_arena(ixtts_gpt* h);
/* A second engine over the SAME device weights (one worker holds a register engine for single sequences / one beam group and a
 * wide engine for several beam groups; the reference has one model object, model_v2.py:433-446): `h` gives up its own arena and
 * reads `owner`'s.  Same model shape and weight type; `owner` must be finalized and outlive `h`. */
int ixtts_gpt_share_arena(ixtts_gpt* h, ixtts_gpt* owner);

/* `store_mel_emb(embeds)` + the prefill forward of generate() for sequence slot `b`
 * (model_v2.py:87-88,144-155): embeds_dev [P-1, D] fp32 = [pad][conds 34][text L+2] rows,
 * attention mask = zeros for the first `n_left_pad` rows then ones (model_v2.py:635-642).
 * Appends the start_mel_token row (mel_embedding[start] + mel_pos[0]) itself, fills the KV
 * cache, resets the slot's history to the fake ids [1]*(P-1)+[start] (model_v2.py:652-661)
 * and leaves the first-step logits ready. */
int ixtts_gpt_prefill(ixtts_gpt* h, int b, const float* embeds_dev, int n_rows, int n_left_pad, void* stream);
/* ixtts_gpt_prefill of n sequences into the n slots `slots[i]` (any slots, any order, none twice) in one packed causal pass per
 * layer: entry i is (slots[i], embeds_dev[i] [n_rows[i], D], n_rows[i], n_left_pad[i]).  Afterwards every named slot holds bit
 * for bit what ixtts_gpt_prefill of its entry alone leaves -- first-step logits, K/V rows, history, prompt_len / valid_from,
 * cleared bans, sequence-bias table and forced ids -- whatever shares the pass and however the call is cut into passes; slots
 * not named are not touched.  A pass holds at most min(rows_max > 0 ? rows_max : max_seq, max_seq) packed rows (the rows
 * workspaces hold max_seq; rows_max exists for tests, production passes 0) and the call makes the passes of
 * ixtts_gpt_prefill_plan.  Every argument is checked before anything is enqueued: 0 <= n <= max_batch (n == 0: no-op), each
 * slot in range and named once, each entry's rows as ixtts_gpt_prefill checks them; IXTTS_ERR_ARG names the entry and the slot
 * and leaves every slot as it was.  Stream-ordered, no host synchronisation of its own.  The tables go down `stream` from one
 * pageable host buffer of the handle, which the next call rewrites: like ixtts_gpt_set_bans and the scalars of
 * ixtts_gpt_prefill, this relies on the HIP runtime having copied (or staged) a pageable source by the time hipMemcpyAsync
 * returns.  The handle has one device copy of the tables and one set of rows workspaces: calls on one handle (this one,
 * ixtts_gpt_prefill, ixtts_gpt_latent) must be ordered by one stream, or by events between streams.  The embeds must stay alive
 * until the stream has consumed them. */
int ixtts_gpt_prefill_many(ixtts_gpt* h, int n, const int* slots, const float* const* embeds_dev, const int* n_rows, const int* n_left_pad,
                           int rows_max, void* stream);
/* The pass rule of ixtts_gpt_prefill_many as a host function (no handle, no GPU): entries in the order given, entry i being
 * n_rows[i] + 1 - n_left_pad[i] packed rows; a pass closes when the next entry would not fit in row_cap rows.  Writes the pass
 * of each entry to pass_of[n] and returns the number of passes (0 for n == 0), IXTTS_ERR_ARG for a null array or row_cap < 1. */
int ixtts_gpt_prefill_plan(const int* n_rows, const int* n_left_pad, int n, int row_cap, int* pass_of);
/* Run up to `n_steps` decode steps for slots [0, n_active): logits -> processors -> token ->
 * embed -> 24 layers.  No host synchronisation inside; a slot that emits stop_mel_token
 * keeps emitting it (generation_utils.py:3255-3256).  Tokens accumulate on the device. */
int ixtts_gpt_decode(ixtts_gpt* h, int n_active, int n_steps, const ixtts_sampler_cfg* sc, void* stream);
/* The same with the sampler settings and the random stream belonging to the SEQUENCE: slot b runs its processors and warpers
 * from per_slot[b] (every field, greedy and sampling slots in one launch included) and draws from
 * uniform(per_slot[b].seed, rng_stream[b], step) -- rng_stream == NULL: the slot index.  ixtts_gpt_decode is the uniform case
 * (every entry *sc, stream = slot index).  A sequence's tokens are a function of its prompt, its entry and its stream: not of
 * the slot it sits in, nor of what the other slots run (on one engine shape; wide and register engines differ in logit bits).
 * Each entry is checked as ixtts_gpt_decode checks *sc; a failure returns IXTTS_ERR_ARG and names the slot.  The arrays are
 * copied before the call returns. */
int ixtts_gpt_decode_slots(ixtts_gpt* h, int n_active, int n_steps, const ixtts_sampler_cfg* per_slot, const uint32_t* rng_stream,
                           void* stream);
/* Synchronises `stream`; returns generated ids of slot b (up to and including the first
 * stop token) and whether the slot has finished. */
int ixtts_gpt_read(ixtts_gpt* h, int b, int32_t* ids_host, int cap, int* n_ids, int* finished, void* stream);
/* Raw fp32 logits of the most recent forward for slot b ([n_mel_codes], device -> host, sync). */
int ixtts_gpt_read_logits(ixtts_gpt* h, int b, float* logits_host, void* stream);
/* Probability vector [n_mel_codes] the last do_sample step drew from for slot b (after penalty,
 * temperature, top-k, top-p, softmax; zeros for removed ids).  Parity-test hook. */
int ixtts_gpt_read_probs(ixtts_gpt* h, int b, float* probs_host, void* stream);
/* `suppress_tokens` / `begin_suppress_tokens` of generate() for the sequence in `slot` (SuppressTokensLogitsProcessor,
 * SuppressTokensAtBeginLogitsProcessor): always_host[n_always] ids are -inf at every step, first_host[n_first] at the first
 * generated token only.  The lists REPLACE the slot's earlier ones; ixtts_gpt_prefill of the slot clears them, so call this after
 * the slot's prefill and before its first decode step.  In beam mode the lists of the group's first slot hold for all its
 * beams.  Stream-ordered (the ids are copied before the call returns); an id outside 0..n_mel_codes-1 returns IXTTS_ERR_ARG. */
int ixtts_gpt_set_bans(ixtts_gpt* h, int slot, const int32_t* always_host, int n_always, const int32_t* first_host, int n_first,
                       void* stream);
/* `sequence_bias` and `bad_words_ids` of generate() for the sequence in `slot` (SequenceBiasLogitsProcessor,
 * NoBadWordsLogitsProcessor): n entries, entry e = the lens_host[e] ids (1..IXTTS_SEQ_BIAS_LEN) that follow those of the entries
 * before it in ids_flat_host, and biases_host[e] (a bad word: -INFINITY; NaN is refused).  A one-id entry adds its bias to that id
 * at every step; a longer one adds it to its last id when the history HF sees -- [1]*(P-1) + [start_mel], then the generated
 * tokens; with beams each beam's own -- ends with its other ids; an entry longer than the history is ignored; entries that end in
 * one id add up.  The bias lands BEFORE the repetition penalty.  n = 0..IXTTS_SEQ_BIAS_MAX; the table REPLACES the slot's earlier
 * one and ixtts_gpt_prefill of the slot clears it, so call this after the prefill; with beams the table of the group's first
 * slot holds for all its beams.  Stream-ordered (copied before the call returns); IXTTS_ERR_ARG names the slot and the limit. */
int ixtts_gpt_set_sequence_bias(ixtts_gpt* h, int slot, const int32_t* ids_flat_host, const int32_t* lens_host, const float* biases_host,
                                int n, void* stream);
/* `forced_eos_token_id` of generate() for the sequence in `slot`: the ids that ixtts_sampler_cfg.forced_eos_step leaves at 0.
 * Replaces the slot's earlier ones, cleared by ixtts_gpt_prefill, the group's first slot with beams -- as ixtts_gpt_set_bans,
 * whose two lists it leaves alone (and which leaves these alone). */
int ixtts_gpt_set_forced_eos(ixtts_gpt* h, int slot, const int32_t* ids_host, int n, void* stream);
/* Teacher forcing for parity tests: overrides the NEXT token chosen for slot b. */
int ixtts_gpt_force_next(ixtts_gpt* h, int b, int32_t token, void* stream);

/* Beam-sample, the reference's served default (`num_beams=3, do_sample=True`: infer_v2.py:598-605) --
 * `_beam_search` + `BeamSearchScorer` (transformers_generation_utils.py:3406-3565, transformers_beam_search.py:215-417,
 * 930-1013) with the whole per-step bookkeeping on the device.  Usage: ixtts_gpt_prefill(h, 0, ...) ->
 * ixtts_gpt_beam_begin(h, num_beams) (beams take slots 0..num_beams-1, needs max_batch >= num_beams) ->
 * ixtts_gpt_beam_decode(h, n_steps, cfg) as often as needed -> ixtts_gpt_beam_read. */
int ixtts_gpt_beam_begin(ixtts_gpt* h, int num_beams, void* stream);
int ixtts_gpt_beam_decode(ixtts_gpt* h, int n_steps, const ixtts_sampler_cfg* sc, void* stream);
/* Synchronises; runs `finalize` (best hypothesis, + eos if it fits in max_new) and returns it.  `done` = the scorer's
 * is_done flag.  Optional outputs (may be NULL): best score, and for tests the open beams' scores [num_beams], their
 * last tokens and the beam_idx of the last step. */
int ixtts_gpt_beam_read(ixtts_gpt* h, int max_new, int32_t* ids_host, int cap, int* n_ids, int* done, float* score,
                        float* beam_scores_host, int32_t* last_tokens_host, int32_t* beam_idx_host, void* stream);
/* Parity-test hook: the NEXT beam step uses these 2*num_beams flat draws (beam*V + token) instead of sampling. */
int ixtts_gpt_beam_force(ixtts_gpt* h, const int32_t* picks_host, int n, void* stream);

/* Beam GROUPS: the reference runs `inference_speech` once per text segment, one after another (infer_v2.py:616-658), each a
 * `_beam_search` over num_beams sequences.  Here the segments of a request (or of several requests) decode TOGETHER: group g
 * owns slots g*num_beams .. g*num_beams+num_beams-1 and its own scorer state (beam scores, hypotheses, done flag, forced
 * draws), the weights are read once per step for all groups.  An engine of up to 4 slots holds one group (the calls above ==
 * group 0); a wide engine (max_batch 5..16, or up to 32 with bf16 / f16 weights) holds floor(max_batch / num_beams) of them.  A group's tokens do not depend
 * on which other groups step with it.  Usage per segment: ixtts_gpt_prefill(h, g*num_beams, ...) ->
 * ixtts_gpt_beam_begin_group(h, g, num_beams, rng_stream) (rng_stream selects the group's random stream: 0 is the stream
 * ixtts_gpt_beam_begin uses, so segment i decoded with rng_stream i draws the same numbers in any group) -> repeated
 * ixtts_gpt_beam_decode_groups(h, n_groups, n_steps, cfg) stepping groups 0..n_groups-1 (finished or parked groups inside
 * that range are no-ops) -> ixtts_gpt_beam_read_group.  ixtts_gpt_beam_park_group takes a group out of the stepping set
 * until its next begin (its slots keep running through the layers with their last token; nothing is read from them). */
int ixtts_gpt_beam_begin_group(ixtts_gpt* h, int group, int num_beams, uint64_t rng_stream, void* stream);
int ixtts_gpt_beam_park_group(ixtts_gpt* h, int group, void* stream);
int ixtts_gpt_beam_decode_groups(ixtts_gpt* h, int n_groups, int n_steps, const ixtts_sampler_cfg* sc, void* stream);
/* The same with one cfg per GROUP (per_group[g], every field: do_sample and length_penalty included; ixtts_gpt_beam_read_group
 * finalizes group g with its own length penalty).  num_beams stays the engine run's.  ixtts_gpt_beam_decode_groups is the
 * uniform case.  Each entry is checked as *sc is; a failure returns IXTTS_ERR_ARG and names the group. */
int ixtts_gpt_beam_decode_groups_cfg(ixtts_gpt* h, int n_groups, int n_steps, const ixtts_sampler_cfg* per_group, void* stream);
int ixtts_gpt_beam_read_group(ixtts_gpt* h, int group, int max_new, int32_t* ids_host, int cap, int* n_ids, int* done, float* score,
                              float* beam_scores_host, int32_t* last_tokens_host, int32_t* beam_idx_host, void* stream);
int ixtts_gpt_beam_force_group(ixtts_gpt* h, int group, const int32_t* picks_host, int n, void* stream);

/* `UnifiedVoice.forward(...)->get_logits(return_latent=True)` (model_v2.py:554-596,486-512):
 * prefix_dev [n_prefix, D] = [conds 34 ; text_emb L+2] rows; codes_dev [n] int32 mel codes.
 * Embeds [start, codes, stop] with mel positions 0..n+1, runs the full causal trunk,
 * ln_f + final_norm, writes the first n mel rows to latent_dev [n, D] fp32. */
int ixtts_gpt_latent(ixtts_gpt* h, const float* prefix_dev, int n_prefix, const int32_t* codes_dev, int n,
                     float* latent_dev, void* stream);
/* ixtts_gpt_latent of n sequences in packed causal passes over the weights: entry i is (prefix_dev[i] [n_prefix[i], D],
 * codes_dev[i] [n_codes[i]]) -> latent_dev[i] [n_codes[i], D], bit for bit what ixtts_gpt_latent of that entry alone writes, for
 * every weight type, whatever else is in the call, in whatever order, under any rows_max.  Any n >= 0 (n == 0: no-op; not bounded
 * by max_batch: like ixtts_gpt_latent the pass runs in the handle's scratch sequence and touches no decode slot, so it may run
 * while slots are in mid-decode); an entry with n_codes == 0 writes nothing.  Every entry is checked as ixtts_gpt_latent checks its
 * arguments before anything is enqueued: IXTTS_ERR_ARG names the entry and leaves every output untouched.  The sequences of a
 * pass share the scratch sequence's cache at disjoint positions, each starting on a multiple of 64 (the key-tile width of the
 * rows attention: only there does a sequence get the tiles, and the rounding, of a pass of its own), and the call makes the
 * passes of ixtts_gpt_latent_plan with row_cap = min(rows_max > 0 ? rows_max : max_seq, max_seq); rows_max exists for tests,
 * production passes 0.  Stream-ordered, no host synchronisation of its own.  The tables of each pass go down `stream` from one
 * pageable host buffer of the handle (its own, not ixtts_gpt_prefill_many's), which the next pass and the next call rewrite: as
 * there, this relies on the HIP runtime having copied (or staged) a pageable source by the time hipMemcpyAsync returns.  One
 * device copy of the tables and one set of rows workspaces per handle: calls on one handle (this one, ixtts_gpt_latent,
 * ixtts_gpt_prefill, ixtts_gpt_prefill_many) must be ordered by one stream, or by events between streams.  Inputs and outputs must
 * stay alive until the stream has consumed them. */
int ixtts_gpt_latent_many(ixtts_gpt* h, int n, const float* const* prefix_dev, const int* n_prefix, const int32_t* const* codes_dev,
                          const int* n_codes, float* const* latent_dev, int rows_max, void* stream);
/* The pass rule of ixtts_gpt_latent_many as a host function (no handle, no GPU): entries in the order given, entry i being
 * T = n_prefix[i] + n_codes[i] rows that occupy ceil(T / 64) * 64 cache positions; a pass closes when the next entry would not fit
 * in row_cap positions (an entry larger than row_cap gets a pass of its own); an entry with n_codes == 0 occupies nothing and
 * takes the pass of its neighbour.  Writes the pass of each entry to pass_of[n] and returns the number of passes (0 for n == 0),
 * IXTTS_ERR_ARG for a null array or row_cap < 1. */
int ixtts_gpt_latent_plan(const int* n_prefix, const int* n_codes, int n, int row_cap, int* pass_of);

/* Microbench hook for bench.py's roofline leg: launches the decode-step GEMV kernel of
 * `which` (0 qkv, 1 attn-out, 2 fc, 3 mlp-out, 4 head) for layer `layer` once on `stream`. */
int ixtts_gpt_bench_gemv(ixtts_gpt* h, int which, int layer, int batch, void* stream);
/* Algorithmic HBM bytes of one decode step at batch B and context S. */
double ixtts_gpt_step_bytes(const ixtts_gpt* h, int B, int S);

/* Largest `max_batch` (decode slots decoded together, weights read once per step for all of them) that EVERY weight type of this
 * build supports: 16. */
int ixtts_gpt_max_batch(void);
/* The same for one weight type: 32 for IXTTS_DTYPE_BF16 and IXTTS_DTYPE_F16 (steps of 17..32 sequences serve two blocks of 16
 * columns from one weight stream), 16 for IXTTS_DTYPE_F32, 0 for anything else.  ixtts_gpt_create refuses more. */
int ixtts_gpt_max_batch_for(int weight_dtype);

int ixtts_gpt_destroy(ixtts_gpt* h);

/* ------------------------------------------------------------------------------------
 * Text emotion model -- Qwen3 causal-LM decode, 1..IXTTS_QWEN_MAX_SLOTS sequences ("slots") per engine
 * replaces: `QwenEmotion.model.generate(...)` (indextts/infer_v2.py:795-906), the arithmetic of
 *   transformers/models/qwen3/modeling_qwen3.py (embed -> L x {RMSNorm, q|k|v, q_norm/k_norm, RoPE, GQA attention,
 *   o_proj + residual, RMSNorm, SiLU(gate) * up, down + residual} -> norm -> lm_head).
 * Weights are f16 (the reference loads torch_dtype="float16") or f32 (parity mode); accumulation, the residual stream,
 * norm statistics and the KV cache are fp32.  Token selection runs on the device: greedy = argmax (lowest id on a tie);
 * sampling = temperature -> top-k -> top-p (HF warper order), 1 <= top_k <= IXTTS_QWEN_TOPK_MAX, draws from the
 * counter-based stream (seed, 0, generated count).
 * Usage: create -> set_tensor (HF names) for every tensor -> finalize -> prefill(prompt ids) -> generate, or step + read.
 * Slots: create_slots(n_slots) -> ... -> prefill_slots(prompts) -> generate_slots, or step_slots, + read_slot per slot.
 *   Slot 0 is the sequence of the one-sequence calls.  One decode step forwards every slot with one pass over the
 *   weights; slot c's logits, kept set and ids are bit for bit those of a one-sequence engine given its prompt alone.
 *   The K/V caches of slots 1.. are allocated by the first prefill_slots of more than one sequence.
 *   f16 engines prefill the prompts of a batch as rows of GEMMs on the f16 matrix cores (activations as two f16 planes,
 *   fp32 accumulation; at most IXTTS_QWEN_ROWS_MAX rows per pass, environment, default 1024 -- lowered by tests);
 *   f32 engines prefill slot after slot exactly as ixtts_qwen_prefill does.
 */
#define IXTTS_QWEN_TOPK_MAX 64
#define IXTTS_QWEN_MAX_EOS 8
#define IXTTS_QWEN_MAX_SLOTS 4

typedef struct ixtts_qwen_cfg {
  int hidden_size;         /* 1024 (multiple of 512) */
  int layers;              /* 28 */
  int heads;               /* 16 query heads */
  int kv_heads;            /* 8 (heads / kv_heads in {1, 2, 4}) */
  int head_dim;            /* 128 (the only value built) */
  int intermediate_size;   /* 3072 (multiple of 512) */
  int vocab_size;          /* 151936 */
  float rms_norm_eps;      /* 1e-6 */
  float rope_theta;        /* 1e6 */
  int tie_word_embeddings; /* lm_head = embed_tokens when lm_head.weight is not given */
  int max_seq;             /* KV-cache positions (prompt + generated) */
  int weight_dtype;        /* IXTTS_DTYPE_F32 | IXTTS_DTYPE_F16 */
  int n_eos;               /* 1..IXTTS_QWEN_MAX_EOS */
  int eos_ids[IXTTS_QWEN_MAX_EOS];
} ixtts_qwen_cfg;

typedef struct ixtts_qwen_sampling {
  int do_sample;     /* 0: argmax */
  float temperature; /* > 0 */
  int top_k;         /* 1..IXTTS_QWEN_TOPK_MAX when do_sample */
  float top_p;       /* (0, 1] */
  uint64_t seed;
} ixtts_qwen_sampling;

typedef struct ixtts_qwen ixtts_qwen;

int ixtts_qwen_create(ixtts_qwen** out, const ixtts_qwen_cfg* cfg); /* = create_slots(out, cfg, 1) */
int ixtts_qwen_create_slots(ixtts_qwen** out, const ixtts_qwen_cfg* cfg, int n_slots);
/* `name` as in the HF state dict (model.embed_tokens.weight, model.layers.N.self_attn.q_proj.weight, ..., lm_head.weight);
 * data_host fp32, converted to the engine's weight dtype.  Synchronous. */
int ixtts_qwen_set_tensor(ixtts_qwen* h, const char* name, const float* data_host, const int64_t* shape, int ndim);
int ixtts_qwen_finalize(ixtts_qwen* h);
/* Resets the sequence to the prompt ids_host[0..n) and runs its first n-1 positions through the layers (1 <= n < max_seq),
 * 4 positions per pass over the weights, the remainder one by one. */
int ixtts_qwen_prefill(ixtts_qwen* h, const int32_t* ids_host, int n, void* stream);
/* n_steps decode steps (each: one position through the model, logits, one token).  A finished sequence (EOS drawn, or
 * the cache full) stays put: further steps change nothing. */
int ixtts_qwen_step(ixtts_qwen* h, int n_steps, const ixtts_qwen_sampling* sc, void* stream);
/* Generated ids so far (EOS included when drawn); *finished: 0 running, 1 EOS, 2 cache full.  Synchronises.  Returns
 * IXTTS_ERR_STATE when a step met non-finite logits (the sequence stopped there without a token). */
int ixtts_qwen_read(ixtts_qwen* h, int32_t* ids_host, int cap, int* n_ids, int* finished, void* stream);
/* Steps until EOS, a full cache or max_new tokens, then reads as ixtts_qwen_read.  Synchronous. */
int ixtts_qwen_generate(ixtts_qwen* h, int max_new, const ixtts_qwen_sampling* sc, int32_t* ids_host, int cap, int* n_ids,
                        int* finished, void* stream);
/* Tests: the fp32 logits [vocab_size] of the last decode step; the ids and probabilities its token selection kept
 * (descending); n draws from those probabilities with stream counters 0..n-1 (the sequence does not move). */
int ixtts_qwen_read_logits(ixtts_qwen* h, float* logits_host, void* stream);
int ixtts_qwen_read_kept(ixtts_qwen* h, int32_t* ids_host, float* probs_host, int cap, int* n_kept, void* stream);
int ixtts_qwen_draw(ixtts_qwen* h, uint64_t seed, int n, int32_t* ids_host, void* stream);
/* HBM bytes of one decode step at context S (weights + K/V rows). */
double ixtts_qwen_step_bytes(const ixtts_qwen* h, int S);
/* Resets slots 0..n-1 to their prompts (ids_host: the prompts one after the other, lens_host[n] their lengths, each
 * 1 <= len < max_seq) and runs each one's first len-1 positions through the layers.  Slots n.. are left as they are. */
int ixtts_qwen_prefill_slots(ixtts_qwen* h, int n, const int32_t* ids_host, const int* lens_host, void* stream);
/* n_steps decode steps of slots 0..n-1 (all prefilled).  A finished slot stays put: it appends no K/V and emits no token. */
int ixtts_qwen_step_slots(ixtts_qwen* h, int n, int n_steps, const ixtts_qwen_sampling* sc, void* stream);
/* Steps slots 0..n-1 until every one is finished or has max_new tokens (the host looks every 16 steps).  Synchronous;
 * read the ids with ixtts_qwen_read_slot. */
int ixtts_qwen_generate_slots(ixtts_qwen* h, int n, int max_new, const ixtts_qwen_sampling* sc, void* stream);
/* ixtts_qwen_read / read_logits / read_kept of one slot. */
int ixtts_qwen_read_slot(ixtts_qwen* h, int slot, int32_t* ids_host, int cap, int* n_ids, int* finished, void* stream);
int ixtts_qwen_read_logits_slot(ixtts_qwen* h, int slot, float* logits_host, void* stream);
int ixtts_qwen_read_kept_slot(ixtts_qwen* h, int slot, int32_t* ids_host, float* probs_host, int cap, int* n_kept, void* stream);
int ixtts_qwen_destroy(ixtts_qwen* h);

/* ---- output stage: requested sample rate and sample encoding, after the vocoder -----------------------------------------------
 * What the reference leaves to its caller: `infer` ends at 22 050 Hz int16 (infer_v2.py:735-783); a deployment that wants 8 kHz
 * G.711 or 16 / 24 / 48 kHz resamples and re-encodes the WAV on its own side.  Here both happen on the device, for every segment
 * of a call in one launch each.
 *
 * Rows: `rows_dev` (int64, device) [n_rows][3] = (src offset, n, dst offset), in elements of the input / output buffer.
 *
 * ixtts_resample_varlen_f32: torchaudio.transforms.Resample(22050, sr) (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) of
 *     n_rows packed fp32 rows of unequal length.  orig / new_ = the two rates over their gcd; output sample j = q * new_ + p of a row
 *     of n samples is sum_k h[p][k] xpad[q * orig + k], xpad = the row behind `width` zeros and zeros after it; a row yields
 *     ceil(n * new_ / orig) samples at y_dev + dst, clamped to +-32767.0.  The tap table arrives as compacted bands (the non-zero
 *     taps of a phase are contiguous in the fp32 table): bands_dev [new_][band | 1] fp32 (row stride band | 1, the whole table
 *     padded to a multiple of 4 floats, 16-byte aligned; bands_elems = floats it holds) with bands[p][k] = h[p][starts[p] + k],
 *     starts_dev (int32) [new_], starts[p] + band <= 2 * width + orig.  max_n = the longest row (it sizes the grid).  A row with
 *     n = 0 writes nothing; a row the buffers cannot hold (src + n > x_elems, dst + ceil(..) > y_elems) is left alone.  A sample
 *     is one fma chain over its own row: the same bits alone, in any batch, at any position.  n_rows <= 65535.
 * ixtts_resample_tile: output samples one workgroup of the resampler produces (IXTTS_RESAMPLE_TILE), for tests that aim at its edges.
 * ixtts_pcm_assemble: out_dev[0 .. total) samples of `encoding`: sample i inside a row's [dst, dst + n) is the conversion of
 *     x_dev[src + i - dst] (fp32 at the +-32767 scale, clamped to the int16 range, truncated toward zero -- `.type(torch.int16)`;
 *     IXTTS_PCM_MULAW / _ALAW: ITU-T G.711 of that int16, one byte, as audioop.lin2ulaw / lin2alaw), every other sample the
 *     encoding's code for silence (0, 0xFF, 0xD5).  Rows ascend in dst and do not overlap.  out_dev is 8-byte aligned and holds
 *     `total` int16 (IXTTS_PCM_S16LE) or bytes.
 * Both run on `stream`, allocate nothing, and return IXTTS_ERR_ARG (text in ixtts_last_error) for a bad shape or an unknown encoding.
 */
#define IXTTS_RESAMPLE_TILE 1024
#define IXTTS_PCM_S16LE 0
#define IXTTS_PCM_MULAW 1
#define IXTTS_PCM_ALAW 2
int ixtts_resample_tile(void);
int ixtts_resample_varlen_f32(const float* x_dev, long x_elems, float* y_dev, long y_elems, const int64_t* rows_dev, int n_rows, long max_n,
                              const float* bands_dev, long bands_elems, const int* starts_dev, int orig, int new_, int width, int band, void* stream);
int ixtts_pcm_assemble(const float* x_dev, long x_elems, void* out_dev, long total, const int64_t* rows_dev, int n_rows, int encoding, void* stream);

/* ---- output stage: programme loudness (ITU-R BS.1770-4) and a sample-peak ceiling -----------------------------------------------
 * The programme of a request is what it delivers: its rows (fp32 at the +-32767 scale) at their offsets, zeros between them, taken
 * as x / 32768.  Tables (device): `rows_dev` int64 [n_rows][3] = (src, n, dst) as above, the rows of a request consecutive and
 * ascending in dst; `reqs_dev` int64 [n_reqs][IXTTS_LOUDNESS_REQ_COLS] = (first row, rows, start, extent, hop, first hop slot): the
 * programme is [start, start + extent) in the coordinate of dst, hop = (fs + 5) / 10 samples, and hop k of the request has slot
 * `first hop slot + k` of the two hop arrays, k < ceil(extent / hop).
 *
 * ixtts_loudness_measure: K-weighting (`coefs_dev` fp64 [n_reqs][IXTTS_LOUDNESS_COEF_COLS] = shelf b0 b1 b2 a1 a2, high-pass a1 a2
 *     with b = 1 -2 1, one unused, then M row-major 4 x 4) over the whole programme from zero state, through the gaps, in fp64;
 *     energy_dev[slot] = the sum of squares of the weighted signal over the hop, hop_peak_dev[slot] = max |x| over it in sample
 *     units (a trailing partial hop gets both over the samples it has).  One wave per hop filters the window from R = hop + hop / 2
 *     samples before the hop (what the filter's slowest pole leaves of a state by then is 1e-14 of it, at every rate) to its end:
 *     a lane filters its chunk of Cw = ceil((R + hop) / 64) | 1 samples from zero state, the chunks' end states are chained with
 *     M = A^Cw -- A the zero-input update of the state (s1, s2, u1, u2) of the two transposed-direct-form-II sections:
 *     s1' = -a1 s1 + s2, s2' = -a2 s1, u1' = -(h1 + 2) s1 - h1 u1 + u2, u2' = (1 - h2) s1 - h2 u1 -- and the lane filters its
 *     chunk again from the state it starts in; the 64 partial sums are added in lane order -- no atomics, a request's numbers are
 *     the same alone and in any launch.  max_hops = the largest
 *     ceil(extent / hop) (it sizes the grid), hop <= IXTTS_LOUDNESS_MAX_HOP, n_reqs <= 65535; a source range outside
 *     [0, x_elems) reads as silence and a slot outside [0, hops_elems) is not written.
 * ixtts_loudness_gain: one workgroup per request, fixed reduction order.  Blocks of 4 hops, z_j = (e_j + .. + e_j+3) / (4 hop),
 *     l_j = -0.691 + 10 log10 z_j, the absolute gate at -70 and the relative gate 10 below the mean of what passed it ->
 *     L (none with fewer than 4 hops or no block above -70).  `targets_dev` fp64 [n_reqs][2] = (target LUFS | NaN: none, ceiling
 *     dBFS | NaN: none).  g = 10^((target - L) / 20) with a target and an L, else 1; with a ceiling c = 32768 * 10^(dBFS / 20) and
 *     g * peak > c, g = c / peak.  records_dev [n_reqs] of ixtts_loudness_record (8-byte aligned): L (NaN: none), g rounded to
 *     fp32 once, the input peak in sample units, flags IXTTS_LOUDNESS_CEILING_BOUND | IXTTS_LOUDNESS_NO_BLOCK, the number of
 *     blocks; gains_dev fp32 [n_reqs] = the same g.
 * ixtts_pcm_assemble_gain: ixtts_pcm_assemble with rows_dev int64 [n_rows][4] = (src, n, dst, gain index): a sample of a row with
 *     0 <= index < n_gains is the conversion of the fp32 product gains_dev[index] * x (one rounding), any other index converts x.
 */
#define IXTTS_LOUDNESS_REQ_COLS 6
#define IXTTS_LOUDNESS_COEF_COLS 24
#define IXTTS_LOUDNESS_MAX_HOP 4800
#define IXTTS_LOUDNESS_CEILING_BOUND 1u
#define IXTTS_LOUDNESS_NO_BLOCK 2u
typedef struct ixtts_loudness_record {
  double lufs;
  float gain;
  float peak;
  uint32_t flags;
  uint32_t blocks;
} ixtts_loudness_record;
int ixtts_loudness_measure(const float* x_dev, long x_elems, const int64_t* rows_dev, int n_rows, const int64_t* reqs_dev, const double* coefs_dev,
                           int n_reqs, long max_hops, double* energy_dev, float* hop_peak_dev, long hops_elems, void* stream);
int ixtts_loudness_gain(const double* energy_dev, const float* hop_peak_dev, long hops_elems, const int64_t* reqs_dev, const double* targets_dev,
                        int n_reqs, ixtts_loudness_record* records_dev, float* gains_dev, void* stream);
int ixtts_pcm_assemble_gain(const float* x_dev, long x_elems, void* out_dev, long total, const int64_t* rows_dev, int n_rows, const float* gains_dev,
                            int n_gains, int encoding, void* stream);

/* ---- output stage: true peak (ITU-R BS.1770 Annex 2) and a look-ahead limiter ---------------------------------------------------
 * Programmes are described as above (`rows_dev`, and for the true peak `reqs_dev`).  Interpolator: `taps` fp64
 * [IXTTS_TRUE_PEAK_TAPS], h[m] = sinc(m / 4) 0.5 (1 + cos(pi m / 24)) at index m + 24; the point n + k / 4 of a programme y is
 * z[4 n + k] = sum_j h[k - 4 j] y[n + j] over the taps that exist (k = 0: the sample; k = 1 .. 3: j = -5 .. 6), fp64 in
 * ascending j over the fp32 samples, zeros outside the programme; points exist for n in [0, extent) only.
 *
 * ixtts_true_peak: hop_peak_dev[slot] = the largest |z| over the points whose n lies in the hop, rounded to fp32 once, for every
 *     programme q with modes_dev[q] == 1 (int64 [n_reqs]; null: every programme) -- the slots `ixtts_loudness_measure` filled with
 *     the sample peak, to be launched between it and `ixtts_loudness_gain`.  One workgroup per hop; max_hops sizes the grid.
 * ixtts_limiter: `lreqs_dev` int64 [n_reqs][IXTTS_LIMITER_REQ_COLS] = (first row, rows, start, extent, offset in out_dev, gain
 *     index, W, offset of the window in tables_dev, mode (1: true), first partial slot), `ceilings_dev` fp64 [n_reqs] = c in sample
 *     units, `tables_dev` fp64 = the taps, then per rate the window w[0 .. 2W], w[k] = 0.5 (1 - cos(2 pi (k + 1) / (2W + 2))) over
 *     its sum; 1 <= W <= IXTTS_LIMITER_MAX_W.  y[n] = fp32(g x[n]) with g = gains_dev[gain index] (an index outside [0, n_gains):
 *     1).  Detector p[n] = |y[n]|, in true mode the max with |z| at n - 3/4 .. n + 3/4; r[n] = min(1, c / p[n]), 1 where p = 0 and
 *     outside [0, extent); m[n] = min over |k| <= W of r[n + k]; a[n] = 1 - sum_k w[k] (1 - m[n - W + k]) in fp64 (<= r[n]: every
 *     m of the sum has n in its window); a32 = fp32(a), one ulp toward zero where that is above r[n]; out_dev[offset + n] =
 *     a32 * y[n], one rounding, for n in [0, extent), gaps included.  One workgroup per tile of IXTTS_LIMITER_TILE samples
 *     (max_tiles sizes the grid); tile t of a programme leaves partials_dev[2 (slot + t)] = the bits of its smallest a32 and
 *     [.. + 1] = its samples with a32 < 1 (uint32; `partial_slots` pairs) for the host to reduce.  out_dev may be another part of
 *     the buffer x_dev points into, disjoint from every row.  A programme its buffers cannot hold is left alone.
 * ixtts_limiter_tile: IXTTS_LIMITER_TILE, for tests that aim at tile edges.
 */
#define IXTTS_TRUE_PEAK_TAPS 49
#define IXTTS_LIMITER_TILE 1024
#define IXTTS_LIMITER_MAX_W 240
#define IXTTS_LIMITER_REQ_COLS 10
int ixtts_limiter_tile(void);
int ixtts_true_peak(const float* x_dev, long x_elems, const int64_t* rows_dev, int n_rows, const int64_t* reqs_dev, const int64_t* modes_dev, int n_reqs,
                    long max_hops, const double* taps_dev, float* hop_peak_dev, long hops_elems, void* stream);
int ixtts_limiter(const float* x_dev, long x_elems, const int64_t* rows_dev, int n_rows, const int64_t* lreqs_dev, const double* ceilings_dev, int n_reqs,
                  long max_tiles, const double* tables_dev, long tables_elems, const float* gains_dev, int n_gains, float* out_dev, long out_elems,
                  uint32_t* partials_dev, long partial_slots, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* IXTTS_HIP_H */
