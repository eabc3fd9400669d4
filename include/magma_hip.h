/*
 * magma_hip.h -- C ABI of libmagma_hip.so (gfx950 / MI355X only).
 *
 * The reference (Aleph-Alpha/magma) has no FFI of its own: its hot path is
 * PyTorch eager ops inside three Python seams:
 *     model.image_prefix(x)                 reference magma/magma.py:208,254
 *     model.word_embedding(ids)             reference magma/magma.py:205,258
 *     model.lm(inputs_embeds|input_ids, use_cache, past_key_values, labels)
 *                                           reference magma/magma.py:270-274,
 *                                           magma/sampling.py:81-93
 * Every entry point below is one fused device computation those seams launch
 * (SURVEY.md 2.4, K1..K24).  The host side (magma_amd/, mirror of the
 * reference's Python surface) binds them with ctypes; INTEGRATION.md shows the
 * stub a reference maintainer would add.
 *
 * Conventions
 *   - all pointers are DEVICE pointers owned by the caller (PyTorch-ROCm
 *     allocations); the library never allocates, frees or synchronises;
 *   - every call only enqueues on `stream` (a hipStream_t passed as void*);
 *     graph-capture safe;
 *   - bf16 = raw uint16 storage; fp32 where stated; ids int64 (torch.long);
 *   - return 0 on success, negative MG_ERR_* otherwise; message via
 *     mg_last_error() (thread local).  Shapes are validated before any launch.
 */
#ifndef MAGMA_HIP_H
#define MAGMA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MG_OK 0
#define MG_ERR_SHAPE (-1)
#define MG_ERR_ALIGN (-2)
#define MG_ERR_HIP (-3)
#define MG_ERR_UNSUPPORTED (-4)
#define MG_ERR_COMM (-5)          /* RCCL missing or an RCCL call failed (mg_comm_*) */

#define MG_ACT_NONE 0
#define MG_ACT_RELU 1
#define MG_ACT_GELU_NEW 2
#define MG_ACT_QUICK_GELU 3 /* x * sigmoid(1.702 x): CLIP ViT MLP */

/* auxiliary-operand modes of the epilogue (backward passes, dropout) */
#define MG_AUX_NONE 0
#define MG_AUX_RELU_GATE 1 /* v *= (aux > 0)            -- ReLU backward            */
#define MG_AUX_GELU_GRAD 2 /* v *= gelu_new'(aux)       -- aux = saved pre-activation */
#define MG_AUX_MUL 3       /* v *= aux                  -- dropout mask (pre-scaled)  */
#define MG_AUX_QUICK_GELU_GRAD 4 /* v *= d/dx [x sigmoid(1.702 x)](aux) -- CLIP ViT MLP backward, aux = saved pre-activation */

/* weight layouts for the B operand of the GEMMs */
#define MG_W_ROWMAJOR 0 /* W[n*ldw + k], k zero-padded to a multiple of 64   */
#define MG_W_FRAGTILED 1 /* [N/16][Kp/32][64 lanes][8]: lane=(kq*16+n%16) holds \
                            W[n][ks*32+kq*8 .. +7]; N padded to 16, Kp to 64 */

#define MG_A_DENSE 0    /* A[m*lda + k]                                       */
#define MG_A_CONV3X3 1  /* A = NHWC image, implicit im2col, pad 1 stride 1    */

typedef uint16_t mg_bf16;

const char* mg_version(void);
/* Binary interface revision.  A binder built against another revision must not call into the library: arguments moved.
 *   1  rounds 1-3.  Within it (before this counter existed) three signatures changed: mg_epilogue._pad became act_n0;
 *      mg_rotary_split_bf16 gained ld_qkv as its 2nd argument; mg_sample_f32's top_p went from float to double.
 *   2  round 4: mg_decode_attn_gemv_bf16 gained ld_attn_out (5th argument), mg_attn_prefill_bf16 gained ld_out (5th), mg_attn_bwd_bf16 /
 *      mg_attn_bwd_merged_bf16 gained ld_o (before the stream); removed: mg_decode_attn_2gemv_bf16,
 *      mg_decode_ctx_counter_ints, the persistent decode step's four entry points mg_decode_plan_* / mg_decode_step_* (in-launch hand-off
 *      experiments, measured slower than the launch chain: DESIGN.md 8).
 *   3  round 5: added mg_stream_create_cu_mask / mg_stream_destroy, mg_rotary_split_fp8 / mg_attn_prefill_fp8 /
 *      mg_attn_fp8_scale_stride (nothing moved; a revision-2 binder keeps working, the loader of this repo asks for 3 because it
 *      binds the new ones).
 *   4  round 5: mg_epilogue grew by C8 / ldc8 / c8_scales / c8_rgroups (the MX e4m3 copy of a tile GEMM's output): every
 *      descriptor that embeds an epilogue changed size.
 *   5  round 6: added mg_rotary_qk_inplace_bf16 / mg_attn_fwd_rows_bf16 / mg_attn_bwd_rows_bf16 (attention without transposed operand
 *      images, q / k / v taken as strided rows -- straight from the fused qkv activation); mg_attn_prefill_fp8 gained
 *      out8 / ld_out8 / out8_scales (the MX e4m3 copy of its output, before the stream).
 *   6  round 6: mg_epilogue.reserved0 became `accumulate` and the struct grew by `row_scale` (weight-gradient GEMMs add
 *      row_scale[m] * (A W^T) straight into the fp32 gradient: no temporary, no second pass): every descriptor that embeds an
 *      epilogue changed size.  Added mg_conv_weight_relayout_batch / mg_bn_fold_batch (one launch per step for all
 *      convolutions of the image encoder) and mg_transpose_bn_param_grad_bf16; mg_rotary_split_fp8 gained `inplace` (before the stream):
 *      the rotated q / k also written back into the fused qkv activation, replacing a mg_rotary_qk_inplace_bf16 pass; mg_attn_bwd_rows_bf16
 *      gained `first_rows` (before the stream): only the gradients of the first positions (the bottom block of a frozen LM).
 *   7  ragged batches (right-padded prompts of different lengths): mg_attn_decode_bf16, mg_attn_decode_fused_bf16,
 *      mg_decode_attn_gemv_bf16 and mg_sample_finish gained `pos_stride` (before the stream; 0 = one KV write position for the
 *      batch as before, 1 = row b at d_pos[b]); mg_advance_pos gained `B` and `pos_stride` (before the stream).
 *   8  beam search: added mg_beam_state, mg_beam_topk_f32, mg_beam_finish and mg_kv_reorder_bf16 (nothing moved).
 *   9  continuing from a cache: mg_rotary_split_bf16 gained `pos_stride` (before the stream; 0 = as before, 1 = row b's chunk starts
 *      at d_pos[b]); added mg_attn_prefill_cached_bf16 (a chunk of new queries per row against the KV cache).
 *  10  logits processors: added mg_logits_process_f32 and mg_beam_topk_scores_f32 (nothing moved).
 *  11  MXFP4 decode weights (W4A16): mg_skinny_desc grew by `w_mx4_scale` at its end (NULL = as before; nothing else moved).
 *  12  per-row stopping: added mg_sample_finish_rows; mg_logits_process_f32 gained `eos_more` / `n_eos_more` (before the stream;
 *      NULL / 0 = as before): further eos ids the min_new_tokens rule bans.
 *  13  transformers' sampler: added mg_sample_warp_f32 (nothing moved).
 *  14  added the test probe mg_debug_mx_mfma_acc (nothing moved).
 *  15  mg_ce_reduce_f32 gained `V` (after R): a target outside [0, V) is ignored by all three cross-entropy kernels alike; before,
 *      the reduction counted every target >= 0 although mg_ce_rows_f32 / mg_ce_bwd_bf16 gave such a row loss 0 and gradient 0.
 *  16  token log-probabilities: added mg_token_logprobs_f32 (nothing moved).
 *  17  constrained decoding: added mg_logits_process_constrained_f32 (nothing moved).
 *  18  classifier-free guidance: added mg_logits_guidance_f32 and mg_guidance_follow (nothing moved).
 *  19  ranking choices: added mg_attn_prefill_tree_bf16, mg_rotary_split_at_bf16 and mg_token_logprobs_rows_f32 (nothing moved).
 *  20  explaining answers: added mg_attn_prefill_scaled_bf16 (nothing moved).
 *  21  diverse beam search: added mg_beam_finish_groups (nothing moved).
 *  22  contrastive search: added mg_contrastive_topk_f32, mg_contrastive_sim_bf16, mg_contrastive_finish and
 *      mg_kv_broadcast_bf16 (nothing moved).
 *  23  losslessly packed decode weights: mg_skinny_desc grew by `pk_lo`, `pk_nib`, `pk_base`, `pk_sign`, `pk_flags` at its end
 *      (NULL = as before; nothing else moved).
 *  24  request streams: added mg_sample_finish_slots and mg_slots_admit_bf16, MG_STOP_LEN and MG_SLOTS_MAX (nothing moved).
 *  25  session prefix of a request stream: added mg_slots_admit_at_bf16 (nothing moved).
 *  26  shared session prefix: added mg_attn_decode_prefix_bf16, mg_attn_decode_fused_shared_bf16, mg_decode_attn_gemv_shared_bf16,
 *      mg_slots_admit_shared_bf16, MG_PREFIX_CHUNK and MG_PREFIX_PART (nothing moved).
 *  27  BatchNorm gain gradient from the convolution output instead of the rounded unit output: added mg_scale_rows_acc_bn_grad_f32
 *      (nothing moved).  Choosing over a request stream: added mg_logits_process_slots_f32,
 *      mg_logits_process_constrained_slots_f32 and mg_token_logprobs_slots_f32 (nothing moved, no revision bump: a package that
 *      binds them names the missing symbol when it meets an older library).  Per-request sampling: added mg_sample_rows_f32 and
 *      MG_SAMPLE_ROW_BYTES, in the same way.  Speculative decoding: added mg_attn_decode_chunk_bf16,
 *      mg_decode_attn_gemv_chunk_bf16 and mg_spec_finish, in the same way.  Speculative decoding for sampled rows and stop
 *      sequences: added mg_sample_chunk_f32 and mg_spec_finish_seq, in the same way. */
#define MG_ABI_VERSION 27
int32_t mg_abi_version(void);
const char* mg_last_error(void);

/* ---- Device-resident indices ------------------------------------------------------------------------------------------------------
 * "Shapes are validated before any launch" covers what the HOST passes.  The token loop never synchronises, so the values that steer
 * addressing inside it live in device memory -- KV positions (d_pos), the step counter (state[0]), tokens and the token history, beam
 * parents, contrastive sources, trie nodes, slot windows -- and no entry point can look at them before the launch.  One rule for every
 * kernel that reads one (DESIGN.md "Device-resident indices" words the same table; tests/test_device_indices_gpu.py holds a case per row):
 *   - a value outside its range is never turned into an address or a table offset: the compare is unsigned or two-sided and is made
 *     before anything is formed from the value, and no signed sum can wrap in front of it;
 *   - SKIP: the row or element the value belongs to is skipped -- nothing of it is written, its output row included, and nothing is
 *     read through it;
 *   - CLAMP, where stated: the value counts as the nearest end of its range, and the table says where the access then lands;
 *   - the other rows of the launch are unaffected, to the bit.
 * The rotary tables sin_t / cos_t are indexed by a guarded position and no kernel knows their row count: they must hold at least Smax
 * rows (the three shared-prefix entry points: n_prefix + Smax rows).
 *
 *   entry point                              value (range)                              outside the range
 *   mg_rotary_split_bf16                     d_pos[0] / d_pos[b] + s  ([0, Smax))       SKIP row s (q_out, K, V and the tables untouched)
 *   mg_rotary_split_at_bf16                  slot d_pos[b] + s, angle row d_pos[b] +    SKIP row s (either one outside)
 *                                            off[b][s]  (each [0, Smax))
 *   mg_attn_decode_bf16, _fused_bf16,        d_pos[b * pos_stride]  ([0, Smax))         SKIP row b: no append, no attention, out row untouched
 *   mg_decode_attn_gemv_bf16                                                            (the co-launched GEMV is unaffected)
 *   mg_attn_decode_chunk_bf16,               d_pos[b * pos_stride] + t  ([0, Smax))     per row t < T of the chunk, the sum formed unsigned: SKIP row
 *   mg_decode_attn_gemv_chunk_bf16                                                      b * T + t alone (no append, no attention, out row untouched)
 *   mg_attn_decode_fused_shared_bf16,        d_pos[b]  ([n_prefix, n_prefix + Smax))    below: CLAMP to n_prefix (own index 0, an idle slot);
 *   mg_decode_attn_gemv_shared_bf16                                                     at or above n_prefix + Smax: SKIP row b
 *   mg_attn_decode_prefix_bf16               d_pos[b]  (as above)                       below: CLAMP to n_prefix.  Above: NOT guarded -- this launch
 *                                                                                       is not told Smax; it rotates q at angle row d_pos[b] and
 *                                                                                       writes partials that the second launch (which skips the
 *                                                                                       row) never reads.  Only `part` rows of b are written.
 *   mg_attn_prefill_cached_bf16, _tree_bf16  d_pos[b * pos_stride]  ([0, Smax])         CLAMP into [0, Smax]; key loads land on slots <= Smax - 1
 *   mg_attn_prefill_tree_bf16                sub[b][j]  ([j + 1, T])                    compared with query indices only, never an index: <= j hides
 *                                                                                       key j from every query, > T counts as T
 *   mg_sample_finish, mg_sample_finish_rows  state[0] as history column ([0, cols))     SKIP the history write; step and positions advance
 *   mg_sample_finish_slots                   state[0], slot[b][0] (any value)           ring: column state[0] mod cols, count in [1, cols]
 *   mg_slots_admit_bf16, _at_bf16,           state[0] (any value)                       ring column (state[0] - 1) mod cols
 *   mg_slots_admit_shared_bf16               first_token[j] (any value)                 stored and compared, never an index.  Rows, slots, lengths,
 *                                                                                       offsets: host arguments, validated before the launch
 *   mg_spec_finish, mg_spec_finish_seq       count[b]  ([0, history_cols])              SKIP row b whole: nothing of it is written, it holds no loop open
 *                                            n_draft[b]  ([0, min(T, token_stride) - 1])  CLAMP; lookup_len[b] CLAMP into [0, lookup_cols]
 *                                            ids, tokens, lookup entries (any value)     compared and stored, never an index; a draft id outside
 *                                                                                       [0, vocab) ends the draft in front of it
 *   mg_logits_process_f32, _constrained_f32  state[0]  ([0, history_cols])              CLAMP: the number of history columns read
 *                                            history tokens, eos / suppress ids ([0,V)) SKIP that id (no penalty, no ban)
 *   mg_logits_process_constrained_f32        roots[r], path[r][i], table entries        a node outside [0, n_nodes): the cache entry is not used /
 *                                                                                       the row is off the trie (eos ids only); edges CLAMP into
 *                                                                                       [0, n_edges]; a header that does not fit table_ints: no trie
 *   mg_token_logprobs_f32                    state[0] as column ([0, cols))             SKIP: nothing written
 *   mg_logits_process_slots_f32,             finish[r][0] >= 0 (idle), slot[r][0]       SKIP row r: logits / lp untouched, no history, root or path
 *   _constrained_slots_f32,                  outside [0, history_cols)                  entry of the row read
 *   mg_token_logprobs_slots_f32              state[0] (any value)                       ring column (state[0] - 1) mod history_cols, count in
 *                                                                                       [1, history_cols]; the lp column = the count: >= cols SKIP
 *                                            tokens, ids, roots, path, table entries    as the flat twins above
 *   mg_sample_rows_f32                       finish[r][0], slot[r][0], state[0]         as the slot twins above: SKIP an idle row (token, filtered
 *                                                                                       untouched, no logit read); the counter is any value
 *                                            record r of params (any bits)              never an index: temperature not finite > 0 = greedy,
 *                                                                                       top_k < 0 = off, top_p / log_min_p NaN or out of range = off
 *   mg_sample_chunk_f32                      finish[b][0] >= 0, count[b]                SKIP the T rows of sequence b (token, filtered untouched, no
 *                                            ([0, history_cols])                        logit read); the counter count[b] + t is any value
 *                                            n_draft[b]  ([0, T - 1])                   CLAMP; rows t above it are SKIPPED
 *                                            record b of params (any bits)              as mg_sample_rows_f32
 *   mg_token_logprobs_f32, _rows_f32         token id ([0, V)), row_of[i] ([0, n_rows)) lp = -inf, nothing read through it
 *   mg_kv_reorder_bf16                       parent[b]  ([0, R))                        SKIP row b (it is then neither staged nor overwritten)
 *                                            d_pos  ([0, Smax])                         CLAMP: the number of positions copied
 *   mg_kv_broadcast_bf16                     src[b]  ([b k, b k + k))                   SKIP the sample
 *                                            d_pos[r] + pos_delta  ([0, Smax))          SKIP row r
 *   mg_beam_finish, mg_beam_finish_groups    cand_tok (any value)                       ranked with, stored and compared, never an index; parents are
 *                                                                                       formed in the launch from list positions, inside the sample
 *                                            state[0]  ([0, ld))                        below 0: no history column gathered or written; >= ld: ld
 *                                                                                       columns gathered, none written
 *   mg_contrastive_sim_bf16                  ctx_len[b]  ([0, Tmax])                    CLAMP: the number of context rows compared
 *   mg_contrastive_finish                    ctx_len[b]  ([0, Tmax))                    SKIP the append, the length stays
 *                                            state[0] as history column ([0, cols))     SKIP the history write
 *   mg_contrastive_topk_f32                  src[b]  ([b k, b k + k))                   CLAMP to row b k
 *   mg_guidance_follow, mg_advance_pos       token, d_pos                               copied / incremented, never an index
 *   mg_embedding_bf16                        ids  ([0, vocab))                          CLAMP: row 0 / row vocab - 1
 *   mg_ce_rows_f32 (mg_ce_reduce_f32,        tgt[r]  ([0, V))                           SKIP: loss 0, gradient 0, not counted, nothing read
 *   mg_ce_bwd_bf16)                                                                                                                      */

/* Fused epilogue shared by both GEMM kernels:
 *   v = acc * scale[n] + bias[n];  C2[m*ldc2+n] = v (optional, bf16: the
 *   pre-activation a later backward pass needs);  v = act(v);
 *   v = aux_op(v, aux[m*ldaux+n]) (unless aux_after);  v += res0 + res1 + res2;
 *   v = aux_op(v, aux) (if aux_after);  v = act_after(v);
 *   C[m*ldc + n] = v  (bf16, or fp32 when out_f32)
 * Covers: Linear(+bias) / gelu_new / adapter ReLU / 3-way GPT-J residual /
 * folded BatchNorm + ReLU / bottleneck "relu(bn3(conv3)+identity)" / dropout /
 * and, in backward, ReLU and GELU gradients fused into the dgrad GEMMs.      */
typedef struct mg_epilogue {
  const float* scale; /* [N] or NULL */
  const float* bias;  /* [N] or NULL */
  int32_t act;        /* MG_ACT_* applied before the residual adds */
  int32_t act_after;  /* MG_ACT_NONE or MG_ACT_RELU, after the residual adds */
  const mg_bf16* res0;
  const mg_bf16* res1;
  const mg_bf16* res2;
  int64_t ldr;        /* row stride of res* (elements) */
  void* C;
  int64_t ldc;
  int32_t out_f32;
  int32_t aux_mode;   /* MG_AUX_* */
  const mg_bf16* aux;
  int64_t ldaux;
  int32_t aux_after;  /* apply the aux op after the residual adds */
  int32_t act_n0;     /* `act` applies to columns n >= act_n0 only (0: all) -- two projections sharing one A in one launch:
                       * [q|k|v | fc_in] with gelu_new on the fc_in columns; multiple of 8 */
  mg_bf16* C2;        /* optional second output (value before `act`), bf16 */
  int64_t ldc2;
  /* optional OCP MX copy of the final value (what C receives, rounded to bf16 first: the same bytes mg_quantize_mx_fp8 makes
   * of the bf16 output): e4m3 elements C8[m * ldc8 + n] with one E8M0 scale per 32 consecutive n in that quantiser's layout
   * (c8_rgroups = ceil(M / 64)) -- the A operand of a following mg_gemm_mx_fp8 without a quantisation pass in between.
   * Tile GEMMs only (mg_gemm_bf16 / mg_gemm_fp8 / mg_gemm_mx_fp8), un-split, N % 32 == 0, ldc8 == ceil(N / 128) * 128,
   * bf16 C (or C == NULL: only the fp8 copy is written).  ABI revision 4.                                              */
  uint8_t* C8;
  int64_t ldc8;
  uint8_t* c8_scales;
  int32_t c8_rgroups;
  /* fp32 outputs only (out_f32): C[m*ldc+n] += v instead of = v -- the weight-gradient GEMMs accumulate into the gradient
   * buffer in place (reference semantics: .grad += over micro-batches, magma/train_loop.py:22-33 through DeepSpeed).  ABI 6.  */
  int32_t accumulate;
  /* optional per-ROW factor of the accumulator, fp32 [M]: v = acc * row_scale[m] * scale[n] + bias[n] (the folded-BatchNorm scale
   * of a convolution's weight gradient: dW[co][:] = scale[co] * g^T a).  Tile GEMMs only; mg_gemm_fp8 takes its activation row
   * scale as an argument instead and refuses both.  ABI 6.                                                                     */
  const float* row_scale;
} mg_epilogue;

/* K9/K11/K12/K13/K14/K18 (GPT-J + adapter GEMMs, prefill/training shapes),
 * K6 (ImagePrefix proj), K2/K3 (CLIP 1x1 / 3x3 convs as implicit GEMM).
 * C[M,N] = A[M,K] * W[N,K]^T, bf16 in, fp32 accumulate, MFMA 16x16x32.
 * Replaces F.linear / F.conv2d calls reached from reference
 * magma/image_prefix.py:83,93 and the LM call at magma/magma.py:270-274.
 *
 * OPERAND SIZE (every entry point of this header): an operand of any size is either addressed correctly or refused with an
 * error, never misread.  Leading dimensions and strides are int64_t and the kernels scale row indices in 64 bits; where a
 * kernel keeps a 32-bit offset, its launcher states the limit and returns MG_ERR_SHAPE past it:
 *   - 256x256 GEMM (tile_hint 0 on large shapes, or 256 ..): the loaders add a 32-bit per-lane byte offset to the workgroup's
 *     64-bit row origin, so 256 rows of A, and of a row-major W, must span less than 2^32 bytes (lda, ldw < 2^23 bf16 elements
 *     / 2^24 fp8 bytes) and a fragment-tiled W less than 2^32 bytes as a whole.  M * lda and N * ldw themselves are not bounded.
 *     Past the limit tile_hint 0 runs the 128x128 kernel (64-bit addresses); a forced 256 tile, and the MX output copy that only
 *     that kernel writes, are refused.
 *   - row attention (mg_attn_fwd_rows_bf16, mg_attn_bwd_rows_bf16): S * ld_row * 2 < 2^31;  cached / tree prefill:
 *     Smax * 256 * 2 < 2^31;  decode attention: Smax <= its stated maximum context.
 * DESIGN.md "Operands past 4 GiB" lists every kernel; tests/test_far_operands_gpu.py holds them to it.                        */
typedef struct mg_gemm_desc {
  const mg_bf16* A;
  int64_t lda;
  const mg_bf16* W;
  int64_t ldw;       /* rowmajor: row stride; fragtiled: padded K (Kp)        */
  int32_t M, N, K;   /* K multiple of 8                                       */
  int32_t a_mode;    /* MG_A_*                                                */
  int32_t w_layout;  /* MG_W_*                                                */
  int32_t H, Wd, Cin; /* conv3x3 only: A is [B,H,Wd,Cin], M = B*H*Wd, K=9*Cin */
  const mg_bf16* zero_page; /* >= 16 zero bytes, 16-B aligned (K/halo padding) */
  mg_epilogue ep;
  int32_t tile_hint; /* 0 = auto; 128 / 256 force the workgroup-tile kernel; 258 / 259: the 256x256 bf16 kernel on the
                      * 32x32x16 / 16x16x32 MFMA (bit-identical, A/B runs); 261..272: timing ablations that exist only in the
                      * ablation build of the library (magma_amd/csrc/Makefile, ABL=1; MG_ERR_UNSUPPORTED otherwise)          */
  int32_t split_k;   /* 0 = auto (only when a workspace is given); 1 = never; n = n-way */
  /* Split-K scratch (optional): small-M GEMMs with a long K (prefill at a few hundred rows,
   * the late CLIP stages) launch fewer tiles than the chip has CUs; with a workspace the
   * library cuts K across several workgroups per tile, each writing an fp32 slab
   * [M][ceil(N/128)*128] here, and a second launch adds the slabs in a fixed order and runs
   * the epilogue (deterministic).  Needs split_k * M * ceil(N/128)*128 * 4 bytes; the
   * library uses fewer splits if it is smaller.  Contents are scratch: do not share one
   * workspace between streams.                                                          */
  float* workspace;
  int64_t workspace_bytes;
} mg_gemm_desc;

int mg_gemm_bf16(const mg_gemm_desc* d, void* stream);
/* Bytes of split-K scratch mg_gemm_bf16 / mg_gemm_fp8 can use for an M x N x K problem at the largest split the automatic
 * policy picks (0 when the shape is never split): what a caller that owns all memory should allocate once.  */
int64_t mg_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K);

/* fp8 operands (BASELINE config 5): A and W hold OCP e4m3 bytes (mg_quantize_rows_fp8), the product
 * runs on v_mfma_scale_f32_16x16x128_f8f6f4 (unit block scales) at twice the bf16 MFMA rate with fp32
 * accumulation, and the epilogue applies  acc * row_scale[m] * ep.scale[n]  (per-row activation scale, per-column
 * weight scale) before bias / activation / residuals.  Same descriptor with every K / lda / ldw counting fp8
 * ELEMENTS: K and lda multiples of 16; row-major W: ldw multiple of 16; fragment-tiled W: the bf16 tiling applied
 * to byte pairs, Kp (ldw) multiple of 128; dense A only; 128x128 tile kernel (split-K as for bf16).  Output
 * bf16 / fp32.                                                                                               */
int mg_gemm_fp8(const mg_gemm_desc* d, const float* row_scale, void* stream);
/* OCP MX (microscaling) form -- BASELINE config 5 as SURVEY 8d states it: e4m3 elements with ONE E8M0 scale per 32 consecutive
 * K-elements of every operand row, multiplied by v_mfma_scale_f32_16x16x128_f8f6f4 with those block scales (no per-row / per-column
 * scale, fp32 accumulate).
 *   mg_quantize_mx_fp8  x [M, K] bf16 -> q [M, ldq] e4m3 in K order (ldq == ceil(K / 128) * 128, zero padded) + the E8M0 block
 *                       scales (shared exponent floor(log2 max|x|) - 8, biased by 127, and ONE HIGHER when the block maximum
 *                       would otherwise exceed 448 -- the v1.0 formula alone saturates maxima in (448, 512) 2^e by up to 12.5 %,
 *                       which the gradient operands of the training path do not tolerate; revision 4) as
 *                       mg_mx_scale_bytes(M, K) bytes: with R = ceil(M / 64), byte ((((k / 128) * 4 + (k / 32) % 4) * R + m / 64) * 16
 *                       + m % 16) * 4 + (m % 64) / 16 is the scale of (row m, block k / 32) -- one dword load hands an MFMA lane
 *                       what it supplies for four 16-row fragments of a 64-row slab (rows >= M of the last slab: unwritten).
 *   mg_gemm_mx_fp8      descriptor as for mg_gemm_fp8 (K / lda / ldw count fp8 elements; rows padded to whole 128-element chunks;
 *                       row-major or fragment-tiled W: the bf16 tiling applied to the byte pairs of the row-major image), the scale
 *                       arrays of the two operands from the quantiser (4-byte aligned).  tile_hint 0 / 128 / 256: the 128x128
 *                       kernel (scales in registers a K-tile ahead; split-K as for bf16) or the 256x256 one (scales staged
 *                       through LDS with their K-tile; bit-identical un-split); the usual epilogue.
 *   mg_debug_mx_mfma    test probe: ONE wave-level MFMA on caller-supplied operand registers (a, b: [64 lanes][8] dwords) and
 *                       per-lane scale dwords -> out [64][4]; pins the instruction's lane / block / scale-byte semantics.
 *   mg_debug_mx_mfma_acc  test probe (revision 14): the same with the accumulator C as an input and for either shape of the
 *                       instruction: form 16 = v_mfma_scale_f32_16x16x128_f8f6f4 (c_in, out [64][4] floats), form 32 =
 *                       v_mfma_scale_f32_32x32x64_f8f6f4 (c_in, out [64][16] floats: the lane's accumulator registers in order);
 *                       out = A B + c_in by ONE instruction of one wave.  Pins how the products of the instruction are aligned,
 *                       truncated and added to C (tests/kernel_compare.py).                                                      */
int64_t mg_mx_scale_bytes(int32_t rows, int32_t K);
int mg_quantize_mx_fp8(const mg_bf16* x, int64_t ldx, int32_t M, int32_t K, uint8_t* q, int64_t ldq, uint8_t* scales, void* stream);
int mg_gemm_mx_fp8(const mg_gemm_desc* d, const uint8_t* a_scales, const uint8_t* w_scales, void* stream);
int mg_debug_mx_mfma(const uint32_t* a, const uint32_t* scale_a, const uint32_t* b, const uint32_t* scale_b, float* out, void* stream);
int mg_debug_mx_mfma_acc(int32_t form, const uint32_t* a, const uint32_t* scale_a, const uint32_t* b, const uint32_t* scale_b,
                         const float* c_in, float* out, void* stream);
/* bf16 rows -> e4m3 rows + one fp32 scale per row (x ~= q * scale[m], scale = rowmax|x| / 448, round to
 * nearest even, saturating); q columns [K, ldq) are zero-filled.  K, ldx, ldq multiples of 8.                */
int mg_quantize_rows_fp8(const mg_bf16* x, int64_t ldx, int32_t M, int32_t K, uint8_t* q, int64_t ldq,
                         float* scale, void* stream);

/* Decode-shape (M <= 16) weight-streaming GEMM: HBM-bound, W must be
 * MG_W_FRAGTILED.  Same epilogue.  Used for every projection of a decode
 * step (reference magma/sampling.py:86-90 -> model.lm(input_ids=...)).       */
typedef struct mg_skinny_desc {
  const mg_bf16* X;
  int64_t ldx;
  const mg_bf16* W;
  int32_t M, N, Kp;  /* Kp = padded K of the tiled weight (multiple of 64)    */
  int32_t nt_hint;   /* 0 = auto; else variant nt | waves<<4 | kc<<8          */
  mg_epilogue ep;
  /* LayerNorm folded into the GEMV: W must already be W*gamma and ep.bias must be
   * b + W.beta; ln_colsum[n] = sum_k W'[n][k].  The kernel derives mean/rstd of each
   * x row from the fragments it streams:  y = rstd*(acc - mean*ln_colsum[n]) + bias[n].
   * NULL = plain GEMV.  (Saves the separate LayerNorm launch of every decode layer.)   */
  const float* ln_colsum;
  float ln_inv_d, ln_eps;
  /* two output segments in one launch (fused qkv | fc_in of a GPT-J block, which share
   * their input): columns [split_n, N) use ep_b (pointers/vectors indexed from column
   * split_n = 0).  0 = single segment.                                                 */
  int32_t split_n;
  int32_t _pad;
  mg_epilogue ep_b;
  /* fp8 weights, bf16 activations (W8A16; halves the weight stream of a decode step).  NULL = bf16 weights.
   * Otherwise W holds e4m3 bytes tiled as [ceil(N/16)][Kp/64][64 lanes][16 B] (lane = kq*16 + n; bytes 0-7 =
   * W[n][64j + 8kq ..+7], bytes 8-15 = W[n][64j + 32 + 8kq ..+7]), w_scale[n] is the per-output-channel scale
   * (W ~= q * w_scale[n]); the kernel widens the bytes to bf16 in registers (exact) and multiplies the
   * accumulators by w_scale before the LayerNorm fold / epilogue.  Needs Kp % 1024 == 0.                     */
  const float* w_scale;
  /* OCP MXFP4 weights, bf16 activations (W4A16; 4.25 bits per weight).  NULL = not MXFP4.  Otherwise W holds e2m1 codes (two per
   * byte, element 2i in the low nibble of byte i) tiled as [ceil(N/16)][Kp/128][64 lanes][16 B] (lane = kq*16 + n; bytes
   * 4s..4s+3 = W[n][128j + 32s + 8kq ..+7], s = 0..3: one 16-byte lane load covers FOUR k-steps) and w_mx4_scale the E8M0
   * block scales, one per 32 K-elements of a row, tiled as [ceil(N/16)][Kp/128][16 n] 32-bit words (byte s of word n = the
   * scale of W[n][128j + 32s .. +31]; value = 2^(byte - 127), bytes in [2, 251]).  One MX block of a row is exactly what one
   * 16x16x32 MFMA step consumes for it: the kernel widens two codes at a time with v_cvt_scalef32_pk_bf16_fp4, the block scale
   * as the scale operand (exact: every e2m1 value times such a power of two is a bf16 value), so nothing is applied after the
   * accumulation.  Rows beyond N are zero.  Needs Kp % 512 == 0, a 16-byte aligned w_mx4_scale, and w_scale == NULL.  ABI 11.   */
  const uint8_t* w_mx4_scale;
  /* Losslessly packed bf16 weights (13.25 bits per weight streamed; every reconstructed bf16 is bit-equal to the one in W, the
   * MFMA sequence is that of the bf16 launch, so the outputs are bit-identical).  pk_lo == NULL = not packed.  Otherwise W stays
   * the bf16 MG_W_FRAGTILED operand and the five arrays hold the same weights again.  A bf16 is s | e[7:0] | m[6:0]; per row n and
   * k-step (32 K-elements: one block) base = min(e>>1), and an element is stored as its low byte (e0<<7 | m), the 4-bit offset
   * (e>>1) - base and its sign.  With j = the k-step quad (128 K-elements), s = the k-step in it, lane = kq*16 + n, element i =
   * W[n][128j + 32s + 8kq + i]:
   *   pk_lo    [ceil(N/16)][Kp/128][2][64 lanes][16 B]  byte 8(s&1) + i of 16-byte group s>>1 = the low byte of element i
   *   pk_nib   [ceil(N/16)][Kp/128][64 lanes][16 B]     byte 4s + b: low nibble = the offset of element b, high nibble of 4 + b
   *   pk_base  [ceil(N/16)][Kp/128][16 n] 32-bit words  byte s = base of row n, k-step 4j + s
   *   pk_sign  [ceil(N/16)][Kp/128][64 lanes] words     bit 8b + 7 - (2s + g) = the sign of element 4g + b of k-step 4j + s
   *   pk_flags [ceil(ceil(N/16)/4)] 32-bit words        byte t&3 of word t>>2 != 0: row tile t is ESCAPED -- one of its blocks
   *            spans more than 16 values of e>>1 (an exact zero beside normal values, a ratio above ~2^30): the workgroups of
   *            such a tile stream W instead (the planes of that tile are not read for values).  Padding bytes are 0.
   * Needs every array 16-byte aligned, Kp % (128 * waves of the variant) == 0 (every Kp % 1024 == 0 fits the automatic choice),
   * and w_scale == w_mx4_scale == NULL.  All five are set or none.  ABI 23.                                                     */
  const uint8_t* pk_lo;
  const uint8_t* pk_nib;
  const uint32_t* pk_base;
  const uint32_t* pk_sign;
  const uint32_t* pk_flags;
} mg_skinny_desc;

int mg_gemm_skinny_bf16(const mg_skinny_desc* d, void* stream);

/* Two independent decode GEMVs in ONE launch (out_proj || adapter-down of a GPT-J block:
 * the 64-workgroup adapter GEMV hides under the other one's weight stream).           */
int mg_gemm_skinny2_bf16(const mg_skinny_desc* a, const mg_skinny_desc* b, void* stream);

/* mg_attn_decode_fused_bf16 co-launched with one GEMV that does not depend on it (fc_out of
 * the parallel block): attention workgroups first, GEMV workgroups behind them, one grid.  */
int mg_decode_attn_gemv_bf16(const mg_bf16* qkv, mg_bf16* kcache, mg_bf16* vcache, mg_bf16* attn_out,
                             int64_t ld_attn_out /* row stride of attn_out in elements; 0 = H*256.  ABI 2: a wider row lets the
                                                  * context land beside another activation, [ctx | t], the input of one K-concatenated
                                                  * GEMV [W_out | W_up] */,
                             int32_t B, int32_t H, int32_t Smax, const int32_t* d_pos, int32_t rot_dim,
                             const float* sin_t, const float* cos_t, const mg_skinny_desc* gemv,
                             int32_t pos_stride /* ABI 7: see mg_attn_decode_fused_bf16 */, void* stream);
/* The same co-launch with the attention workgroups in the shared-prefix mode (ABI 26: mg_attn_decode_fused_shared_bf16 below); the
 * GEMV runs the variant mg_decode_attn_gemv_bf16 picks for the same operand. */
int mg_decode_attn_gemv_shared_bf16(const mg_bf16* qkv, mg_bf16* kcache, mg_bf16* vcache, mg_bf16* attn_out, int64_t ld_attn_out,
                                    int32_t B, int32_t H, int32_t Smax, const int32_t* d_pos, int32_t rot_dim, const float* sin_t,
                                    const float* cos_t, const mg_skinny_desc* gemv, int32_t pos_stride, int32_t n_prefix,
                                    const float* part, void* stream);

/* K8/K17 + ImagePrefix LN: y = (x-mean)/sqrt(var+eps)*gamma+beta, fp32 stats.  Replaces nn.LayerNorm at reference
 * magma/image_prefix.py:58-60,106-107 and ln_1 / ln_f of the GPT-J blocks built at magma/language_model.py:12-45
 * (arithmetic in the un-vendored transformers fork).                                                        */
int mg_layernorm_bf16(const mg_bf16* x, int64_t ldx, const float* gamma, const float* beta,
                      mg_bf16* y, int64_t ldy, int32_t rows, int32_t d, float eps, void* stream);

/* K7: out[b*out_bstride + (row_off+t)*d .. ] = wte[ids[b*T+t]]
 * (reference magma/magma.py:205,258; writes straight into the concatenated
 * [prefix|text] buffer, replacing torch.cat at magma.py:212,261-267).        */
int mg_embedding_bf16(const int64_t* ids, int32_t B, int32_t T, const mg_bf16* wte, int32_t vocab,
                      int32_t d, mg_bf16* out, int64_t out_bstride, int32_t row_off, void* stream);

/* K9 epilogue (the fork's GPT-Neo attention with rotary=True, jax=True, configured at reference
 * magma/language_model.py:17-24; called through magma/magma.py:270-274): split fused qkv rows, GPT-J interleaved rotary on the first
 * rot_dim dims of q,k, scatter K,V into the cache, optional V^T for prefill.
 *   qkv [B*S, 3*H*256];  q_out [B,H,S,256];  kcache/vcache [B,H,Smax,256];
 *   vt (nullable) [B,H,vt_ld/32,256,32] (values transposed in 32-key tiles, vt_ld % 32 == 0);  position of row s = pos0 + s where
 *   pos0 = d_pos ? *d_pos : pos0_host.  sin/cos tables [n_pos, rot_dim/2] f32, n_pos >= Smax.  pos0_host + S > Smax is refused; a
 *   device position is guarded in the kernel, in both forms: a row s with pos0 + s outside [0, Smax) is skipped ("Device-resident indices") */
int mg_rotary_split_bf16(const mg_bf16* qkv, int64_t ld_qkv /* row stride in elements, 0 = 3*H*256 */, int32_t B, int32_t S, int32_t H, int32_t rot_dim,
                         const float* sin_t, const float* cos_t, int32_t pos0_host,
                         const int32_t* d_pos, mg_bf16* q_out, mg_bf16* kcache, mg_bf16* vcache,
                         int32_t Smax, mg_bf16* vt, int32_t vt_ld,
                         int32_t pos_stride /* ABI 9: 0 = positions from pos0 as above; 1 = row b's row s at d_pos[b] + s (d_pos
                                             * required, vt NULL; slots at or past Smax are skipped) */, void* stream);

/* Training form of K9 (positions 0..S-1): q, k, v [B,H,S,256] plus ALL THREE column-tiled transposes vt, qt, kt
 * [B,H,ld_t/32,256,32] in one pass over qkv -- vt feeds mg_attn_prefill_bf16, qt / kt are the s-contraction operands
 * of mg_attn_bwd_bf16 (otherwise two more mg_head_transpose_bf16 passes in the backward).                          */
int mg_rotary_split_train_bf16(const mg_bf16* qkv, int32_t B, int32_t S, int32_t H, int32_t rot_dim,
                               const float* sin_t, const float* cos_t, mg_bf16* q, mg_bf16* k, mg_bf16* v,
                               mg_bf16* vt, mg_bf16* qt, mg_bf16* kt, int32_t ld_t, void* stream);

/* K10 prefill/training forward (same attention module; reference call sites magma/magma.py:270-274 and the
 * prefill step magma/sampling.py:81-85): causal flash attention, head dim 256, fp32
 * online softmax, scale 1/16.  q [B,H,S,256]; k rows from kcache [B,H,Smax,256];
 * vt [B,H,vt_ld/32,256,32]; out [B*S, H*256].  lse (nullable) [B,H,S] fp32.         */
int mg_attn_prefill_bf16(const mg_bf16* q, const mg_bf16* kcache, const mg_bf16* vt, mg_bf16* out,
                         int64_t ld_out /* row stride of out in elements; 0 = H*256 (ABI 2: see mg_decode_attn_gemv_bf16) */,
                         float* lse, int32_t B, int32_t H, int32_t S, int32_t Smax, int32_t vt_ld,
                         void* stream);

/* K10 with a per-key scale on the score (ABI 20; DESIGN.md "Explaining an answer"): the operands of mg_attn_prefill_bf16 plus
 * key_scale, fp32, row b's S entries at key_scale + b * ld_scale (ld_scale >= S floats; the heads of a row share it).  For query t and
 * key j of row b the score is  s[t][j] = (q_t . k_j) / 16 * key_scale[b][j]  in fp32, the causal mask (j > t excluded) is applied
 * AFTER the scaling, then the fp32 softmax and P V of mg_attn_prefill_bf16.  A scale of 0 therefore leaves the key the weight
 * exp(0 - max), a masked key stays masked whatever its scale, and the running maximum is taken over the scaled scores.  lse is the
 * log-sum-exp of the scaled scores.  Entries must be finite and >= 0 (the caller's duty: the kernel does not look); nothing past
 * key_scale[b][S - 1] is read.  One implementation, the 32-query-wave kernel that mg_attn_prefill_bf16 runs by default (its
 * MAGMA_ATTN_FWD switch does not apply here): with key_scale == 1 out and lse have that kernel's bits.  ld_out % 8 == 0 (0 = H*256),
 * S <= 4096 (the row's scales are staged in LDS), key_scale 4-byte aligned.                                                         */
int mg_attn_prefill_scaled_bf16(const mg_bf16* q, const mg_bf16* kcache, const mg_bf16* vt, mg_bf16* out, int64_t ld_out,
                                float* lse, int32_t B, int32_t H, int32_t S, int32_t Smax, int32_t vt_ld,
                                const float* key_scale, int64_t ld_scale, void* stream);

/* K10 over a cache (ABI 9): causal flash attention of a chunk of T new queries per sequence against the KV cache, the arithmetic of
 * mg_attn_prefill_bf16 (fp32 online softmax, scale 1/16).  Row b's chunk starts at p_b = d_pos[b * pos_stride] (pos_stride as in
 * mg_attn_decode_bf16); query t sits at position p_b + t and attends to cache keys [0, p_b + t] -- the chunk's own K / V must already be
 * written at [p_b, p_b + T) (mg_rotary_split_bf16 with pos_stride).  q: rotated queries, row t of head (b, h) at
 * q + b q_stride_b + h q_stride_h + t q_ld_row (elements, multiples of 8; [B,H,T,256]: 256, H T 256, T 256); kcache / vcache
 * [B,H,Smax,256] read as rows (no V^T); out [B*T, >= H*256] at row stride ld_out (0 = H*256).  Key loads stay below
 * min(p_b + T, Smax); rows t >= T_b of a right-padded chunk compute values nobody reads.                                              */
int mg_attn_prefill_cached_bf16(const mg_bf16* q, int64_t q_ld_row, int64_t q_stride_b, int64_t q_stride_h,
                                const mg_bf16* kcache, const mg_bf16* vcache, mg_bf16* out, int64_t ld_out, int32_t B, int32_t H,
                                int32_t T, int32_t Smax, const int32_t* d_pos, int32_t pos_stride, void* stream);

/* K10 over a cache, the chunk a TREE (ABI 19; DESIGN.md "Ranking choices"): mg_attn_prefill_cached_bf16 with another mask.  The
 * chunk's T rows are the non-root nodes of a trie in depth-first preorder; sub [B, T] int32 (row stride T), sub[b][j] = one past
 * the last row of node j's subtree, so "j is t or an ancestor of t" is j <= t < sub[b][j].  Query t of row b sees the cache keys
 * [0, p_b) and chunk key j (cache slot p_b + j) iff j <= t && t < sub[b][j]; the chunk's K / V must already be written at
 * [p_b, p_b + T) (mg_rotary_split_at_bf16).  sub[b][j] == T for every j is a chain: the causal mask, and the bytes of
 * mg_attn_prefill_cached_bf16.  Padding rows of a ragged batch carry sub[b][t] = t + 1 (they see the prompt and themselves).
 * Every other operand is mg_attn_prefill_cached_bf16's, laid out as there.  p_min: the caller's HOST copy of the smallest p_b
 * (d_pos lives on the device and the call only enqueues): every query must see at least one cached key, so p_min < 1 is
 * refused with MG_ERR_SHAPE before the launch, as are a NULL sub and strides that are no multiples of 8.  Key loads stay below
 * min(p_b + T, Smax).                                                                                                          */
int mg_attn_prefill_tree_bf16(const mg_bf16* q, int64_t q_ld_row, int64_t q_stride_b, int64_t q_stride_h,
                              const mg_bf16* kcache, const mg_bf16* vcache, mg_bf16* out, int64_t ld_out, int32_t B, int32_t H,
                              int32_t T, int32_t Smax, const int32_t* d_pos, int32_t pos_stride, const int32_t* sub, int32_t p_min,
                              void* stream);

/* K9 for such a chunk (ABI 19): mg_rotary_split_bf16 with pos_stride = 1 and the slot and the angle apart.  d_pos [B] and
 * off [B, S] int32 (row stride S): row s of sequence b is written to cache slot d_pos[b] + s and rotated with the angles of
 * position d_pos[b] + off[b][s] (a trie node: off = depth - 1).  qkv [B*S, >= 3*H*256] at row stride ld_qkv (0 = 3*H*256);
 * q_out [B,H,S,256]; kcache / vcache [B,H,Smax,256]; sin / cos tables [>= Smax, rot_dim/2] f32.  A row whose slot or position lies
 * outside [0, Smax) is skipped.  off[b][s] == s gives the bytes of mg_rotary_split_bf16 with pos_stride = 1.                       */
int mg_rotary_split_at_bf16(const mg_bf16* qkv, int64_t ld_qkv, int32_t B, int32_t S, int32_t H, int32_t rot_dim,
                            const float* sin_t, const float* cos_t, const int32_t* d_pos, const int32_t* off, mg_bf16* q_out,
                            mg_bf16* kcache, mg_bf16* vcache, int32_t Smax, void* stream);

/* K10 decode (reference magma/sampling.py:86-90, past_key_values path): one query row per (b,h) against
 * ctx = pos_b + 1 cached keys, pos_b = d_pos[b * pos_stride].
 * pos_stride (ABI 7): 0 = one position for the whole batch (d_pos[0]); 1 = d_pos holds B positions, one per row (a ragged,
 * right-padded batch: row b's prompt has its own length, its cache slots >= pos_b are never read before a step writes them). */
int mg_attn_decode_bf16(const mg_bf16* q, const mg_bf16* kcache, const mg_bf16* vcache,
                        mg_bf16* out, int32_t B, int32_t H, int32_t Smax, const int32_t* d_pos,
                        int32_t pos_stride, void* stream);

/* K9 epilogue + K10 decode in ONE launch: takes the fused qkv row of the new token
 * [B, 3*H*256], rotates q,k at angle row pos_b, appends k,v at pos_b, attends over [0, pos_b];
 * pos_b = d_pos[b * pos_stride] as in mg_attn_decode_bf16.  A pos_b outside [0, Smax) skips the row in all three decode entry
 * points: nothing is appended, nothing attended over, the output row stays ("Device-resident indices" above).                 */
int mg_attn_decode_fused_bf16(const mg_bf16* qkv, mg_bf16* kcache, mg_bf16* vcache, mg_bf16* out, int32_t B,
                              int32_t H, int32_t Smax, const int32_t* d_pos, int32_t rot_dim,
                              const float* sin_t, const float* cos_t, int32_t pos_stride, void* stream);

/* Chunk decode attention (DESIGN.md "Speculative decoding"): mg_attn_decode_fused_bf16 for T consecutive positions of every
 * sequence, 2 <= T <= 8, in one launch that reads the sequence's K/V once.  qkv is [B*T, 3*H*256], sequence-major: row b*T + t is the
 * t-th new token of sequence b and sits at position p = pos_b + t, pos_b = d_pos[b * pos_stride]; the caches are [B, H, Smax, 256];
 * out is [B*T, >= H*256] at row stride ld_out (0 = H*256).  Row t is live iff (unsigned)p < Smax; a dead row appends nothing, attends
 * over nothing and leaves its out row as it is.  All live rows' q and k are rotated at their own angle rows, k and v appended at
 * [pos_b, pos_b + T), then query t attends over keys [0, pos_b + t].  Grid B*H workgroups of 256 threads; query t is column t of the
 * score MFMA's B operand, softmax and PV are formed per query in the single-query kernel's order, so out and both caches have the
 * BITS of T successive mg_attn_decode_fused_bf16 launches over the same sequences with row t fed at position pos_b + t (finite K/V).
 * The score area lives in dynamic LDS, T * (Smax * 4 + 4656) bytes: T = 8 at Smax = 2048 takes 100 KB of the 160 KB of a workgroup.
 * Refused before any launch: what mg_attn_decode_fused_bf16 refuses, T outside [2, 8], B*T > 16, an ld_out that is neither 0 nor a
 * multiple of 8 >= H*256, a T and Smax whose LDS does not fit (MG_ERR_SHAPE).  (Added without a revision bump, as mg_sample_rows_f32
 * was: a package that binds it names the missing symbol when it meets an older library.)
 * mg_decode_attn_gemv_chunk_bf16: mg_decode_attn_gemv_bf16 for such a chunk, ONE launch -- B*H attention workgroups that run the chunk
 * body above, and the workgroups of one independent GEMV over an M = B*T operand in the instantiation mg_decode_attn_gemv_bf16 picks
 * for the same descriptor, so the GEMV has that launch's bits.  The grid's LDS block is dynamic, max(the chunk body's, the GEMV's), and
 * every workgroup gets it; the GEMV workgroups also carry the chunk bodies' register count (DESIGN.md "Speculative decoding" has what
 * that does to their occupancy).  Every refusal of either part -- mg_attn_decode_chunk_bf16's, the descriptor's, a K of the GEMV that
 * is no multiple of 128 -- comes before the launch. */
int mg_attn_decode_chunk_bf16(const mg_bf16* qkv, mg_bf16* kcache, mg_bf16* vcache, mg_bf16* out, int64_t ld_out, int32_t B, int32_t T,
                              int32_t H, int32_t Smax, const int32_t* d_pos, int32_t rot_dim, const float* sin_t, const float* cos_t,
                              int32_t pos_stride, void* stream);
int mg_decode_attn_gemv_chunk_bf16(const mg_bf16* qkv, mg_bf16* kcache, mg_bf16* vcache, mg_bf16* attn_out, int64_t ld_attn_out, int32_t B,
                                   int32_t T, int32_t H, int32_t Smax, const int32_t* d_pos, int32_t rot_dim, const float* sin_t,
                                   const float* cos_t, const mg_skinny_desc* gemv, int32_t pos_stride, void* stream);

/* Decode attention over ONE prefix shared by all rows (ABI 26; DESIGN.md "Shared session prefix").  Every row b <= 16 of the batch has
 * the same n_prefix cached positions in front of its own: they are stored once, kprefix / vprefix [H, S_prefix, 256] (positions
 * [0, n_prefix) are read), and the rows' caches [B, H, Smax, 256] hold their OWN positions only -- absolute position p >= n_prefix of a
 * row at own index p - n_prefix.  d_pos stays absolute (the rotary angle); a d_pos[b] < n_prefix counts as n_prefix, a d_pos[b] >=
 * n_prefix + Smax skips the row in the second launch ("Device-resident indices" above; the tables hold n_prefix + Smax rows).  Two launches:
 * mg_attn_decode_prefix_bf16: grid H x n_chunk, n_chunk = ceil(n_prefix / MG_PREFIX_CHUNK) -- a function of n_prefix alone.  Workgroup
 *   (h, c) rotates q of all B rows of the fused qkv [B, 3*H*256] (each at its own position), scores the chunk's keys against all of
 *   them with one set of K loads (row b = MFMA column b) and writes, per row, the chunk's maximum m, sum l = sum exp(s - m) and
 *   o = sum exp(s - m) v (fp32, unnormalised): part[((b*H + h)*n_chunk + c)*MG_PREFIX_PART + {0..255: o, 256: m, 257: l}].  Keys >=
 *   n_prefix of the last chunk are masked.  `part` holds B*H*n_chunk*MG_PREFIX_PART floats.  Nothing of rows >= B is read or written.
 * mg_attn_decode_fused_shared_bf16: mg_attn_decode_fused_bf16 on the own positions -- k, v appended at own index d_pos[b] - n_prefix,
 *   attention over own keys [0, d_pos[b] - n_prefix] -- merged with the row's partials in ascending chunk order under one maximum and
 *   rounded to bf16 once.  A chunk whose weight underflows contributes an exact 0.
 * Refused before any launch: B > 16, n_prefix outside [1, 4096], S_prefix < n_prefix, Smax outside [1, 4096], pos_stride != 1, null or
 * misaligned (16-byte) pointers, rot_dim not a multiple of 8 in [0, 256]. */
#define MG_PREFIX_CHUNK 64
#define MG_PREFIX_PART 264
int mg_attn_decode_prefix_bf16(const mg_bf16* qkv, const mg_bf16* kprefix, const mg_bf16* vprefix, float* part, int32_t B, int32_t H,
                               int32_t n_prefix, int32_t S_prefix, const int32_t* d_pos, int32_t rot_dim, const float* sin_t,
                               const float* cos_t, int32_t pos_stride, void* stream);
int mg_attn_decode_fused_shared_bf16(const mg_bf16* qkv, mg_bf16* kcache, mg_bf16* vcache, mg_bf16* out, int32_t B, int32_t H,
                                     int32_t Smax, const int32_t* d_pos, int32_t rot_dim, const float* sin_t, const float* cos_t,
                                     int32_t pos_stride, int32_t n_prefix, const float* part, void* stream);

/* K24 greedy (reference magma/sampling.py:96-97, temperature == 0.0): token[b] = argmax_v logits[b, v] (first maximum), int64 out;
 * optionally appends to out_tokens[b*out_ld + *d_pos_out] and bumps *d_pos.  */
int mg_argmax_f32(const float* logits, int64_t ld, int32_t B, int32_t V, int64_t* token,
                  void* stream);
/* d_pos[0] += delta (pos_stride 0), or d_pos[b] += delta for b < B (pos_stride 1, ABI 7). */
int mg_advance_pos(int32_t* d_pos, int32_t delta, int32_t B, int32_t pos_stride, void* stream);

/* K24 sampled (reference magma/sampling.py:99-107: top_k_filter :22-30, top_p_filter :7-19 -- the reference's own rule, SURVEY Q6 --
 * softmax(logits / temperature), multinomial) as one launch per token step, graph-capturable (csrc/sampling.hip).
 *   logits [B, V] fp32 (row stride ld); top_k == 0 / top_p == 0 disable the respective filter; top_p is a DOUBLE: the reference
 *   compares fp32 probabilities with the Python scalar (1 - threshold), i.e. with fp32(double(1) - double(threshold));
 *   seed  device uint64 (read at run time: a new seed needs no re-capture), state device int32[2] = {step, first step at which
 *   every row produced eos (-1 until then)}: the random stream is Philox4x32-10 keyed by the seed at counter (step, row);
 *   token [B] int64 sampled ids (NULL: filter only); filtered [B, V] optional copy of the filtered logits (-inf where the
 *   reference's filters put -inf).
 * mg_sample_finish is the loop bookkeeping of a token step in one small launch: records the first step with
 * (token == eos).all() (reference sampling.py:109, read by the host every few steps instead of a sync per token), advances
 * the step counter, bumps the KV-cache write position by delta (d_pos NULL: untouched; pos_stride 0: d_pos[0]; 1: all B
 * entries d_pos[b], ABI 7) and appends the tokens to
 * history[b * ld_history + step] (NULL: off; the host copies the history once when generate() ends); `clear` (NULL: off) =
 * n_clear int32 at clear[i * clear_stride] set to zero for the next step (device-side counters a caller wants re-armed
 * inside the captured step).                                                                                             */
int mg_sample_f32(const float* logits, int64_t ld, int32_t B, int32_t V, float temperature, int32_t top_k, double top_p,
                  const uint64_t* seed, const int32_t* state, int64_t* token, float* filtered, int64_t ld_filtered,
                  void* stream);
/* transformers' sampler (ABI 13; DESIGN.md "transformers' sampler"): mg_sample_f32's launch with the rules of transformers'
 * TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper (min_tokens_to_keep = 1) in place of the
 * reference's filters, then the same draw on the same Philox stream (host statements: magma_amd/sampling.py top_k_filter_ties,
 * nucleus_filter, min_p_filter).  Arguments as mg_sample_f32, plus min_p; the temperature must be > 0 also for a filter-only call,
 * because the nucleus is cut from the probabilities at that temperature.
 *   top_k   every logit below the k-th largest goes; every tie AT the k-th value stays (0 or >= V: off);
 *   top_p   with q the 2^-40 fixed-point probabilities of the top-k survivors at the temperature, total their sum and
 *           c = (uint64)((double)(float)(1 - top_p) * 2^40): a token stays iff the mass ranked before it (descending) is below
 *           max(total - c, 1); of equal logits at the boundary the first ones by index stay (0 or 1: off);
 *   min_p   a token stays iff x >= max + temperature * log(min_p), i.e. p >= min_p * p_max (0: off);
 *   the first maximum always stays; -inf entries carry no mass and are never selected.                                        */
int mg_sample_warp_f32(const float* logits, int64_t ld, int32_t B, int32_t V, float temperature, int32_t top_k, double top_p,
                       double min_p, const uint64_t* seed, const int32_t* state, int64_t* token, float* filtered,
                       int64_t ld_filtered, void* stream);
/* Per-request sampling (DESIGN.md "Per-request sampling"): the launch of mg_sample_f32 (warp = 0) or mg_sample_warp_f32 (warp = 1)
 * -- one workgroup per row, enqueue-only, graph-capturable, no allocation, no scratch, nothing shared between workgroups -- in
 * which every row has its own temperature, top_k, top_p, min_p and seed, read at run time from a device table: another request's
 * settings replay the same captured graph.  It is the same kernel body compiled with another source for its scalars, so for
 * equal logits bits row r's token and filtered row are those of the flat call on that row ALONE (B = 1) with the row's scalars
 * and seed at state[0] = j -- whichever row, and whatever the other rows hold.
 *   params  device table of R records of MG_SAMPLE_ROW_BYTES = 32 bytes, 16-byte aligned:
 *             offset  0  double   top_p        as mg_sample_f32 / mg_sample_warp_f32 take it
 *             offset  8  double   log_min_p    log(min_p) in double as mg_sample_warp_f32 forms it on the host (the C library's
 *                                              log), -inf = off.  The LOGARITHM is stored so that the row's bound max + T log(min_p)
 *                                              has the flat call's bits; read only with warp = 1.
 *             offset 16  uint64   seed         the Philox4x32-10 key of the row
 *             offset 24  float    temperature  0 = the row is greedy: the first maximum, as mg_argmax_f32; it reads no seed
 *             offset 28  int32    top_k        0 or >= V: off
 *   counter the draw of row r uses counter {j, 0, 0, 0}, j = the row's own token index.  slot == NULL (a static call: all rows
 *           start together): j = state[0].  Otherwise (a slot session; slot, finish, history_cols as in
 *           mg_token_logprobs_slots_f32): j = the occupant's token count before this step, (state[0] - 1) mod history_cols - begin
 *           mod history_cols + 1 -- the n - 1 of mg_sample_finish_slots, which runs behind this launch --, and a row whose finish
 *           record says finished / idle, or whose begin lies outside the ring, is SKIPPED: none of its logits is read (they may be
 *           NaN), its token and filtered row are left alone.
 *   token   [R] int64 (NULL: filter only); filtered optional [R, V] (row stride ld_filtered): -inf where a rule dropped the token;
 *           a greedy row keeps its first maximum alone.
 * The table's values cannot be validated here: a temperature that is NaN, negative, zero or infinite selects greedily, a negative
 * top_k is off, a top_p outside (0, 1) or NaN is off, a NaN log_min_p is off; no value of a record forms an address.
 * Refused before anything is launched: R <= 0, V <= 0, ld < V, ld_filtered < V, warp outside {0, 1}, a null logits / params / state,
 * token and filtered both null, finish without slot or slot without finish, slot with history_cols <= 0, params not 16-byte
 * aligned, an fp32 / int32 pointer not 4-byte or token not 8-byte aligned.  (Added without a revision bump, as the slot entry
 * points of 27 were: a package that binds it names the missing symbol when it meets an older library.) */
#define MG_SAMPLE_ROW_BYTES 32
int mg_sample_rows_f32(const float* logits, int64_t ld, int32_t R, int32_t V, int32_t warp, const void* params,
                       const int32_t* state, const int32_t* slot, const int32_t* finish, int32_t history_cols, int64_t* token,
                       float* filtered, int64_t ld_filtered, void* stream);

/* The selection launch of a speculative step (DESIGN.md "Speculative decoding"): a third source for the same kernel body, both
 * warp values -- one workgroup per fed row r = b * T + t of logits [B * T, V], enqueue-only, graph-capturable, no allocation, no
 * scratch.
 *   params  the table of mg_sample_rows_f32, ONE record per sequence: fed row r reads record b = r / T
 *   count   int32 [B]: mg_spec_finish's count, read before that launch updates it.  The draw of row r uses counter
 *           {count[b] + t, 0, 0, 0} under the record's seed: the index token[r] has in sequence b's own stream when the drafts in
 *           front of it were right, which is the only case mg_spec_finish keeps it in.  T = 1 with count[b] = 0 is the arming
 *           call's selection from the prefill logits.
 *   n_draft int32 [B] or NULL (= 0); finish int32 [B][2] and history_cols as mg_spec_finish takes them
 * Row r is SKIPPED whole -- none of its logits read (they may be NaN), token[r] and filtered row r left alone -- if finish[b][0] >= 0,
 * count[b] lies outside [0, history_cols], or t > clamp(n_draft[b], 0, T - 1): the rows mg_spec_finish never reads.  For equal
 * logits bits a live row's token and filtered row are those of mg_sample_rows_f32 on that one row with params[b] and state[0] =
 * count[b] + t; a greedy record takes the first maximum.  No value of a record, of count or of n_draft forms an address unclamped.
 * Refused before anything is launched: as mg_sample_rows_f32 (B for R), and T outside [1, 8], B * T > 16, a null count or finish,
 * history_cols < 0.  (Added without a revision bump, as mg_sample_rows_f32 was.) */
int mg_sample_chunk_f32(const float* logits, int64_t ld, int32_t B, int32_t T, int32_t V, int32_t warp, const void* params,
                        const int32_t* count, const int32_t* n_draft, const int32_t* finish, int32_t history_cols, int64_t* token,
                        float* filtered, int64_t ld_filtered, void* stream);
int mg_sample_finish(const int64_t* token, int32_t B, int64_t eos, int32_t* state, int32_t* d_pos, int32_t delta,
                     int64_t* history, int64_t ld_history, int32_t history_cols, int32_t* clear, int32_t n_clear,
                     int32_t clear_stride, int32_t pos_stride, void* stream);

/* Per-row stopping (ABI 12; DESIGN.md "Per-row stopping"): mg_sample_finish's bookkeeping with the stopping rule of transformers'
 * GenerationMixin._sample -- a row that finished stays finished and is padded, the loop ends when no row is unfinished -- several
 * eos ids and stop sequences, in ONE enqueue-only, graph-capturable launch of one workgroup (host statement:
 * magma_amd/sampling.py, stop_update).  token, B, state, d_pos, delta, history, clear and pos_stride as in mg_sample_finish.
 *   table   device int32[MG_STOP_TABLE_INTS] = eos ids [8] | sequence lengths [16] | sequence tokens [16][16]; read at run time
 *           (other ids of the same counts need no re-capture); n_eos in [1, 8] and n_seq in [0, 16] are launch arguments.
 *   finish  device int32 [B][2] = {step at which the row finished (-1: unfinished), reason}; reason = MG_STOP_EOS | i (token ==
 *           eos id i) or MG_STOP_SEQ | j (the row's tokens history[b][0 .. step] end with sequence j, the lowest such j); eos is
 *           tested first.  The caller resets it to {-1, 0} when a loop starts.
 * Per row, with step = state[0]: a finished row gets `pad` written into token[b] (the next step feeds it back) and into
 * history[b][step]; an unfinished row's token goes into the history and is tested.  Then state[1] = step if no row is unfinished
 * and state[1] < 0; state[0] = step + 1; d_pos advanced.  Any B (rows are strided over the workgroup).  A sequence only matches
 * while step < history_cols, and a length outside [1, 16] or above step + 1 never matches: nothing outside the history is read.
 * n_seq > 0 without a history is refused.                                                                                    */
#define MG_STOP_MAX_EOS 8
#define MG_STOP_MAX_SEQ 16
#define MG_STOP_MAX_LEN 16
#define MG_STOP_TABLE_INTS (MG_STOP_MAX_EOS + MG_STOP_MAX_SEQ + MG_STOP_MAX_SEQ * MG_STOP_MAX_LEN)
#define MG_STOP_EOS 0x100
#define MG_STOP_SEQ 0x200
int mg_sample_finish_rows(int64_t* token, int32_t B, int32_t* state, int32_t* d_pos, int32_t delta, int64_t* history,
                          int64_t ld_history, int32_t history_cols, int32_t* clear, int32_t n_clear, int32_t clear_stride,
                          int32_t pos_stride, const int32_t* table, int32_t n_eos, int32_t n_seq, int64_t pad, int32_t* finish,
                          void* stream);

/* Speculative greedy decoding (DESIGN.md "Speculative decoding"; host statement: magma_amd/sampling.py, speculate_update): the
 * bookkeeping of a step that fed T tokens per sequence, in ONE enqueue-only, graph-capturable launch of one workgroup, B*T <= 16.
 *   ids        int64 [B][T]: the tokens the step fed -- ids[b][0] the last emitted token, ids[b][1 .. n_draft[b]] the drafts; rewritten
 *              for the next step (unused entries repeat ids[b][0]; a finished row holds the pad id table[0])
 *   token      int64: token[b * token_stride + t] = the argmax of fed row t (token_stride = T), or the prefill's selected token with
 *              token_stride = 1 and n_draft = 0: the arming call, which records token 0 and makes the first drafts
 *   history    int64 [B][ld_history], count int32 [B]: the row's emitted tokens and their number
 *   finish     int32 [B][2] = {count at which the row finished or -1, reason}; table: the stop table (eos ids 0 .. n_eos - 1)
 *   lookup     int32 [B][ld_lookup], lookup_len int32 [B]: ids searched in front of the history (lookup_cols may be 0)
 *   stats      int32 [B][3] = {launches in which the row was open, drafts fed, drafts accepted}
 * Per unfinished row: a = the leading j in [1, n_draft] with ids[b][j] == token[b][j - 1]; the tokens token[b][0 .. a] are emitted, cut
 * behind the first eos id among them (MG_STOP_EOS | i) and at limit - count (MG_STOP_LEN; history_cols bounds limit); the m emitted
 * tokens go to history[b][count ..], count += m, d_pos[b] += m (d_pos may be NULL: the arming call feeds nothing).  A row that stays
 * open gets drafts by transformers' prompt-lookup rule over lookup[b][:lookup_len[b]] ++ history[b][:count]: for n from
 * min(max_ngram, L - 1) down to 1, the first window from the left that equals the last n tokens and has a continuation inside the
 * sequence gives at most num_tokens drafts, cut in front of the first eos id (or id outside [0, vocab)); the first n with a match
 * decides.  A finished row is frozen: n_draft = 0, ids = pad, nothing recorded, its position stays.  state[1] latches the step
 * (state[0]) at which no row is open; state[0] += 1.  Refused: null or misaligned pointers, T outside [2, 8], B*T > 16, token_stride
 * other than 1 or T, num_tokens outside [1, T - 1], max_ngram outside [1, 16], n_eos outside [1, 8], bad history / lookup geometry. */
int mg_spec_finish(int64_t* ids, int32_t B, int32_t T, int32_t* n_draft, const int64_t* token, int32_t token_stride, int64_t* history,
                   int64_t ld_history, int32_t history_cols, int32_t* count, int32_t* finish, const int32_t* table, int32_t n_eos,
                   int32_t limit, int32_t* d_pos, const int32_t* lookup, int64_t ld_lookup, int32_t lookup_cols,
                   const int32_t* lookup_len, int32_t* stats, int32_t* state, int32_t num_tokens, int32_t max_ngram, int32_t vocab,
                   void* stream);
/* mg_spec_finish with stop sequences: the same kernel (mg_spec_finish is it at n_seq = 0).  table is the full MG_STOP_TABLE_INTS
 * table of mg_sample_finish_rows, n_seq in [0, 16] of its sequences live.  Every emitted token j is recorded at
 * history[b][count + j], then tested: eos ids first, then every sequence against the tail of history[b][:count + j + 1] -- only this
 * call's tokens, a sequence longer than that never matches -- the lowest matching index winning with MG_STOP_SEQ | i.  The finishing
 * token is kept and emission is cut behind it: stop_update's rule token by token.  Drafts are still cut only in front of eos ids; a
 * draft that completes a sequence is accepted and the row finishes.  (Added without a revision bump.) */
int mg_spec_finish_seq(int64_t* ids, int32_t B, int32_t T, int32_t* n_draft, const int64_t* token, int32_t token_stride,
                       int64_t* history, int64_t ld_history, int32_t history_cols, int32_t* count, int32_t* finish,
                       const int32_t* table, int32_t n_eos, int32_t n_seq, int32_t limit, int32_t* d_pos, const int32_t* lookup,
                       int64_t ld_lookup, int32_t lookup_cols, const int32_t* lookup_len, int32_t* stats, int32_t* state,
                       int32_t num_tokens, int32_t max_ngram, int32_t vocab, void* stream);

/* Request streams (ABI 24; DESIGN.md "Request streams"; host statement: magma_amd/sampling.py, slot_update): the bookkeeping of a
 * slot session, in which the row of a finished request is handed to the next request while the other rows keep generating.
 * mg_sample_finish_slots: mg_sample_finish_rows' launch (one workgroup, enqueue-only, graph-capturable, any B; the same table, pad
 *   and finish record) with
 *     slot    device int32 [B][2] = {begin, limit}: the history column of the occupant's first token and its max_new_tokens.  The
 *             occupant's own token count at a step is n = (step % history_cols - begin) mod history_cols + 1.  A stop sequence of
 *             length l matches only if n >= l: tokens of the previous occupant never take part.  A row that reaches n >= limit
 *             without an eos or stop match finishes with reason MG_STOP_LEN | 0.
 *     history a RING: the column of a step is step % history_cols, for the write and for the stop-sequence reads, so a session
 *             runs for any number of steps.  Required, with 0 < history_cols <= ld_history.
 *     d_pos   one position per row (pos_stride 1).  Only a row that is still open AFTER this step advances by delta: a finished
 *             row stays at a written position while it idles.  Its token and history column get `pad`.
 *   state[1] latches the first step at which no row is open; state[0] advances.
 * mg_slots_admit_bf16: n <= min(B, MG_SLOTS_MAX) staged requests installed into slots, in one launch outside the captured step.
 *   kstage / vstage [L, n_stage, H, S_stage, 256] are the staging caches, kcache / vcache [L, B, H, Smax, 256] the live ones.
 *   src_row, dst_slot, len, limit are HOST arrays of n entries, first_token a DEVICE array of n tokens.  For every j: K and V
 *   positions [0, len[j]) of every layer and head of staging row src_row[j] are copied to live row dst_slot[j] (16-byte vectors,
 *   64-bit offsets); d_pos[slot] = len[j]; token[slot] = first_token[j]; slot[slot] = {c, limit[j]} with c = (state[0] - 1) %
 *   history_cols; history[slot][c] = first_token[j]; the row test runs on the first token (eos, stop sequences of length 1, then
 *   limit[j] <= 1) and leaves finish[slot] = {state[0] - 1, code} or {-1, 0}.  state[1] = -1.  A session starts with state = {1, -1}.
 *   Refused: a duplicate dst_slot, a slot or staging row out of range, len outside [1, min(S_stage, Smax)], n > B or > MG_SLOTS_MAX.
 * mg_slots_admit_at_bf16 (ABI 25; DESIGN.md "Request streams", session prefix): mg_slots_admit_bf16 behind pos0 cached positions
 *   that every staging row and every live slot already hold.  For every j, K and V positions [pos0, pos0 + len[j]) of staging row
 *   src_row[j] go to the SAME positions of live row dst_slot[j], and d_pos[slot] = pos0 + len[j]; positions below pos0 are neither
 *   read nor written.  Token, window, history column, row test, finish record and state[1] are mg_slots_admit_bf16's; one kernel
 *   serves both (mg_slots_admit_bf16 is pos0 = 0).  Refused in addition, before anything is launched: pos0 < 0, len[j] < 1,
 *   pos0 + len[j] > min(S_stage, Smax).
 * mg_slots_admit_shared_bf16 (ABI 26; DESIGN.md "Shared session prefix"): the same launch with a destination offset of its own, for a
 *   live cache that holds the rows' own positions only.  Staged positions [pos0, pos0 + len[j]) go to live positions
 *   [dst0, dst0 + len[j]); d_pos[slot] = pos0 + len[j], the absolute position.  Each side is checked against its own extent: refused
 *   are pos0 outside [0, S_stage), dst0 outside [0, Smax), len[j] < 1, pos0 + len[j] > S_stage, dst0 + len[j] > Smax.  With dst0 = pos0
 *   it is mg_slots_admit_at_bf16. */
#define MG_STOP_LEN 0x300
#define MG_SLOTS_MAX 16
int mg_sample_finish_slots(int64_t* token, int32_t B, int32_t* state, int32_t* d_pos, int32_t delta, int64_t* history,
                           int64_t ld_history, int32_t history_cols, int32_t* clear, int32_t n_clear, int32_t clear_stride,
                           int32_t pos_stride, const int32_t* table, int32_t n_eos, int32_t n_seq, int64_t pad, int32_t* finish,
                           const int32_t* slot, void* stream);
int mg_slots_admit_bf16(const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage, mg_bf16* kcache,
                        mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n, const int32_t* src_row,
                        const int32_t* dst_slot, const int32_t* len, const int64_t* first_token, const int32_t* limit,
                        int32_t* state, int32_t* d_pos, int64_t* token, int32_t* finish, int32_t* slot, int64_t* history,
                        int64_t ld_history, int32_t history_cols, const int32_t* table, int32_t n_eos, int32_t n_seq, void* stream);
int mg_slots_admit_at_bf16(const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage, mg_bf16* kcache,
                           mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n, const int32_t* src_row,
                           const int32_t* dst_slot, const int32_t* len, const int64_t* first_token, const int32_t* limit,
                           int32_t* state, int32_t* d_pos, int64_t* token, int32_t* finish, int32_t* slot, int64_t* history,
                           int64_t ld_history, int32_t history_cols, const int32_t* table, int32_t n_eos, int32_t n_seq,
                           int32_t pos0, void* stream);
int mg_slots_admit_shared_bf16(const mg_bf16* kstage, const mg_bf16* vstage, int32_t n_stage, int32_t S_stage, mg_bf16* kcache,
                               mg_bf16* vcache, int32_t L, int32_t B, int32_t H, int32_t Smax, int32_t n, const int32_t* src_row,
                               const int32_t* dst_slot, const int32_t* len, const int64_t* first_token, const int32_t* limit,
                               int32_t* state, int32_t* d_pos, int64_t* token, int32_t* finish, int32_t* slot, int64_t* history,
                               int64_t ld_history, int32_t history_cols, const int32_t* table, int32_t n_eos, int32_t n_seq,
                               int32_t pos0, int32_t dst0, void* stream);

/* Beam search (transformers' GenerationMixin._beam_search, do_sample=False, one eos id; DESIGN.md "Beam search"): three
 * enqueue-only, graph-capturable launches per token step over R = B * k rows (k = num_beams <= 16, rows sample-major).
 * mg_beam_topk_f32: per row, the top K2 = 2k candidate scores run[row] + log_softmax(logits[row]) in the order (score
 *   descending, lower token first) -> cand_score [R, K2] fp32, cand_tok [R, K2] int32.  Needs 2 <= K2 <= min(32, V)
 *   (diverse beam search asks for K2 = k + k / G).
 * mg_beam_finish: per sample, the top 2k of the k*V candidates (merge of its rows' lists by score descending, then lower flat
 *   index beam*V + token), then the finish / next-beam / early-stop rules: candidates among the first k that end in eos (or
 *   reach max_steps) finish with score sum / gen_len^length_penalty and merge into the k finished slots; the best k that do not
 *   become the running beams (parent[row], token[row] = the fed-back token, run[row]); histories gathered by parent; d_pos
 *   advanced (pos_stride 0: d_pos[0]; 1: all R entries); state = {step, first step at which generation stops} as in
 *   mg_sample_finish.  early_stopping: 0 = False (heuristic on the current length), 1 = True, 2 = "never".
 * mg_kv_reorder_bf16: for every row b with p = parent[b] != b, K / V positions [0, d_pos[p * pos_stride]) of row p (its
 *   positions before this call) copied into row b, every layer and head; positions of b past that are left alone (caches
 *   [L, R, H, Smax, 256]; kstage / vstage of the same shape hold the rows that are read by another row and are themselves
 *   overwritten).  Two launches; any parent map within [0, R), on uniform and per-row positions.
 *   mg_beam_finish writes identity parents at every step after the recorded stop (the finished slots are final then).        */
typedef struct mg_beam_state {
  float* run;           /* [R] running-beam scores (in/out)                                                     */
  float* fin_score;     /* [R] finished-slot scores, sample-major (k slots per sample)                          */
  int32_t* fin_flag;    /* [R] 1 = the slot holds a finished hypothesis                                         */
  int32_t* fin_len;     /* [R] generated length of the slot's hypothesis (eos included)                         */
  int64_t* fin_tok;     /* [R, ld] tokens of the finished hypotheses (eos after fin_len)                        */
  int64_t* fin_stage;   /* [R, ld] staging copy                                                                 */
  int64_t* hist;        /* [R, ld] token history of the running beams                                           */
  int64_t* hist_stage;  /* [R, ld] staging copy                                                                 */
  int64_t ld;           /* columns of the four token buffers                                                    */
  int32_t* unsat;       /* [B] ([B * G] with groups) the early-stop heuristic still allows an improvement (latched) */
  int32_t* parent;      /* [R] out: the row each new running row continues                                      */
  int64_t* token;       /* [R] out: the new last token of each running row                                      */
} mg_beam_state;
int mg_beam_topk_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const float* run, int32_t K2, float* cand_score,
                     int32_t* cand_tok, void* stream);
int mg_beam_finish(const float* cand_score, const int32_t* cand_tok, int32_t B, int32_t k, int32_t V, int64_t eos,
                   double length_penalty, int32_t early_stopping, int32_t max_steps, int32_t* state, int32_t* d_pos,
                   int32_t pos_stride, const mg_beam_state* bs, void* stream);
/* Diverse beam search (ABI 21; Vijayakumar et al. 2018; DESIGN.md "Diverse beam search"; host statement: magma_amd/sampling.py,
 * group_beam_search): mg_beam_finish for k beams in G groups of k' = k / G (rows sample-major, then group-major: row
 * b*k + g*k' + q).  A group is a sample of k' beams in every rule above: its own running scores, k' finished slots and
 * early-stop latch (unsat has B*G entries, index b*G + g); the stop of the call is mg_beam_finish's over the B*G groups.  Within a
 * step the groups of a sample are handled in the order g = 0 .. G-1, and group g's candidate scores are
 * cand_score - diversity_penalty * n_t in fp32 (one rounded product, one rounded subtraction, no fma), n_t = the number of running
 * beams of groups 0 .. g-1 of that sample whose token selected at this step is t; -inf stays -inf.  cand_score / cand_tok
 * [R, K2] are mg_beam_topk_f32's (or mg_beam_topk_scores_f32's) lists of length K2 = k + k' -- at most k - k' tokens are
 * penalised, so no token outside a row's unpenalised top k + k' reaches the group's top 2k' -- or 2k at G = 1, where the call
 * writes what mg_beam_finish writes, bit for bit.  One workgroup, the device code of mg_beam_finish.
 * Needs 1 <= G <= k, k % G == 0, K2 as above, k' * K2 <= 512, V >= K2, diversity_penalty finite and >= 0.                  */
int mg_beam_finish_groups(const float* cand_score, const int32_t* cand_tok, int32_t B, int32_t k, int32_t G, int32_t K2,
                          float diversity_penalty, int32_t V, int64_t eos, double length_penalty, int32_t early_stopping,
                          int32_t max_steps, int32_t* state, int32_t* d_pos, int32_t pos_stride, const mg_beam_state* bs,
                          void* stream);
int mg_kv_reorder_bf16(mg_bf16* kcache, mg_bf16* vcache, mg_bf16* kstage, mg_bf16* vstage, int32_t L, int32_t R, int32_t H,
                       int32_t Smax, const int32_t* parent, const int32_t* d_pos, int32_t pos_stride, void* stream);

/* Logits processors (ABI 10; DESIGN.md "Logits processors"): transformers' RepetitionPenaltyLogitsProcessor,
 * NoRepeatNGramLogitsProcessor, MinNewTokensLengthLogitsProcessor and SuppressTokensLogitsProcessor, applied in that order, in
 * place, to the fp32 rows logits [R, ld] (columns >= V untouched) in ONE enqueue-only launch of one workgroup per row; no
 * allocation, no scratch.  step = state[0] (device) tokens have been generated; row r's are history[r * ld_history + 0 .. len),
 * len = min(step, history_cols).
 *   repetition_penalty p > 0 (1 = off): every DISTINCT token t of the row's history, once: x[t] = x[t] < 0 ? x[t] * p : x[t] / p
 *     (fp32 multiply / correctly rounded divide);
 *   no_repeat_ngram n in [0, 16] (0 = off): if len >= n, every window start w in [0, len - n] whose n - 1 tokens equal the last
 *     n - 1 tokens sets x[history[w + n - 1]] = -inf (n = 1: every generated token);
 *   min_new_tokens: step < min_new_tokens sets x[eos] = -inf, and x[eos_more[i]] = -inf for i < n_eos_more <= 8 (ABI 12; device
 *     int32, NULL / 0 = one eos id as before);   suppress [n_suppress <= 1024] int32 (device): x[t] = -inf.
 * Token ids outside [0, V) -- in the history, eos, the suppress list -- are skipped.  history may be NULL when neither the
 * penalty nor the n-gram rule is on.  V is bounded by the LDS token map of the penalty (491 520).
 * normalize = 1 (beam search): first x <- (x - max) - logsumexp over the V columns, with the arithmetic mg_beam_topk_f32 uses
 * internally (the same bits), then the rules -- not renormalised afterwards, as in transformers' _beam_search.
 * mg_beam_topk_scores_f32 is mg_beam_topk_f32 for rows that already hold such scores: candidates run[row] + scores[row][t].  */
int mg_logits_process_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state, const int64_t* history,
                          int64_t ld_history, int32_t history_cols, float repetition_penalty, int32_t no_repeat_ngram,
                          int32_t min_new_tokens, int64_t eos, const int32_t* suppress, int32_t n_suppress, int32_t normalize,
                          const int32_t* eos_more, int32_t n_eos_more, void* stream);
int mg_beam_topk_scores_f32(const float* scores, int64_t ld, int32_t R, int32_t V, const float* run, int32_t K2,
                            float* cand_score, int32_t* cand_tok, void* stream);

/* Constrained decoding (ABI 17; DESIGN.md "Constrained decoding"; host statement: magma_amd/sampling.py, constrain_logits):
 * mg_logits_process_f32's launch -- its rules first, with its arguments; there is no beam form -- after which row r keeps only the
 * tokens that continue the walk of its history through a token trie; every other column in [0, V) becomes -inf, a kept column
 * keeps its value.  Still ONE enqueue-only launch of one workgroup per row: no allocation, no scratch, no host round trip.
 * table (device int32 [table_ints], read at run time -- the counts too, so a captured launch follows whatever the buffer holds) is
 * a forest of tries over token ids; node ids are indices into its arrays, which follow each other without gaps:
 *   [0] n_nodes >= 1   [1] n_edges
 *   first[n_nodes + 1]    node i's edges are e in [first[i], first[i + 1]);  first[0] = 0, first[n_nodes] = n_edges
 *   terminal[n_nodes]     != 0: a listed sequence ends at the node (every leaf is terminal)
 *   parent[n_nodes]       the node the edge into i leaves, -1 for a root
 *   in_token[n_nodes]     the token of the edge into i (-1 for a root)
 *   edge_token[n_edges]   ascending within a node, distinct within a node
 *   edge_child[n_edges]
 * so table_ints >= 3 + 4 n_nodes + 2 n_edges.  roots [R] (device int32): the root of row r's trie.  With len = min(state[0],
 * history_cols), the row walks history[r * ld_history + 0 .. len) from roots[r], following the edge of each token:
 *   the walk ends at node i   kept: the tokens of i's edges, and -- if terminal[i] -- eos and eos_more[0 .. n_eos_more);
 *   the walk leaves the trie  (a token that is no edge of the node it is at; it never returns): kept: the eos ids alone.
 * Token ids outside [0, V) are skipped everywhere; nothing beyond history_cols is read; history may not be NULL.  A header or a root
 * that does not fit (counts < 0, 3 + 4 n + 2 e > table_ints, root outside [0, n_nodes)) counts as off the trie, and every index
 * an entry supplies is bounded by the header before it is used.
 * path (device int32 [R, MG_TRIE_MAX_LEN], any contents; rows belong to the launch while it runs): a cache of the nodes the walk
 * passed, path[r][i] = the node after i + 1 tokens.  An entry is used only after parent / in_token have shown it to be that node
 * for THIS table and history, so stale or foreign contents never change a result; the launch rewrites the entries it walks.  */
#define MG_TRIE_MAX_LEN 64
int mg_logits_process_constrained_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state, const int64_t* history,
                                      int64_t ld_history, int32_t history_cols, float repetition_penalty, int32_t no_repeat_ngram,
                                      int32_t min_new_tokens, int64_t eos, const int32_t* suppress, int32_t n_suppress,
                                      const int32_t* eos_more, int32_t n_eos_more, const int32_t* table, int64_t table_ints,
                                      const int32_t* roots, int32_t* path, void* stream);

/* The three launches above for the rows of a slot session (DESIGN.md "Choosing over a request stream"; host statement of the
 * window: magma_amd/sampling.py, slot_tokens): each takes its flat twin's arguments, then slot [R][2] = {begin, limit} and finish
 * [R][2] = {step or -1, code} -- the tables mg_sample_finish_slots keeps (device int32, read at run time) --, and
 * mg_token_logprobs_slots_f32 also the ring's column count, which its twin has no argument for.  history is the RING
 * [R, ld_history >= history_cols] and is never optional.  Per row r, with s = state[0]:
 *   idle      finish[r][0] >= 0 (finished and not harvested, or never occupied), or begin outside [0, history_cols): the row is
 *             skipped -- its logits keep their bits, no lp / top column is written, nothing of its history, root or path is read;
 *   occupied  the occupant has n = (((s - 1) mod history_cols) - begin) mod history_cols + 1 tokens, token i at ring column
 *             (begin + i) mod history_cols: the twin's row with len = n, step = n (min_new_tokens compares n) over exactly these
 *             columns -- across the wrap, never a column outside the window --, the same bits as the twin gives on the unrolled
 *             window with state[0] = n.  The log-probability launch writes column n of row r (column 0 is the admission's);
 *             n >= cols writes nothing.
 * path keeps its prove-before-trust rule: what the slot's previous occupant or another table left fails the proof.
 * Enqueue-only, graph-capturable, one workgroup per row, no allocation, no scratch.                                            */
int mg_logits_process_slots_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state, const int64_t* history,
                                int64_t ld_history, int32_t history_cols, float repetition_penalty, int32_t no_repeat_ngram,
                                int32_t min_new_tokens, int64_t eos, const int32_t* suppress, int32_t n_suppress, int32_t normalize,
                                const int32_t* eos_more, int32_t n_eos_more, const int32_t* slot, const int32_t* finish,
                                void* stream);
int mg_logits_process_constrained_slots_f32(float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* state,
                                            const int64_t* history, int64_t ld_history, int32_t history_cols,
                                            float repetition_penalty, int32_t no_repeat_ngram, int32_t min_new_tokens, int64_t eos,
                                            const int32_t* suppress, int32_t n_suppress, const int32_t* eos_more, int32_t n_eos_more,
                                            const int32_t* table, int64_t table_ints, const int32_t* roots, int32_t* path,
                                            const int32_t* slot, const int32_t* finish, void* stream);
int mg_token_logprobs_slots_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const int64_t* token, const int32_t* state,
                                float* lp, int64_t ld_lp, int32_t cols, int32_t n_top, int32_t* top_id, float* top_lp,
                                const int32_t* slot, const int32_t* finish, int32_t history_cols, void* stream);

/* Classifier-free guidance (ABI 18; DESIGN.md "Classifier-free guidance"; host statement: magma_amd/sampling.py, guide_logits):
 * the rule of transformers' UnbatchedClassifierFreeGuidanceLogitsProcessor with the plausibility cut of contrastive decoding, in
 * ONE enqueue-only, graph-capturable launch of one workgroup per pair of rows; no allocation, no scratch.  cond [R, ld_cond] and
 * uncond [R, ld_uncond] fp32; columns >= V of either are neither read nor written, uncond is only read.  Per pair, in place on the
 * conditional row, with c = log_softmax(cond row), u = log_softmax(uncond row) -- each (x - m) - log sum_v exp(x[v] - m), m the row
 * maximum, maximum and sum of BOTH rows from one sweep over the pair (online form) --:
 *   cond[i] = u[i] + scale * (c[i] - u[i])
 *   cond[i] = -inf   where the old cond[i] is -inf, or (old cond[i] - m_cond) < log_min_p   (fp32 comparison on the RAW logits;
 *                    log_min_p = -inf: no cut; the row maximum always stays, ties at the bound stay)
 * scale finite and >= 0 (1: the conditional log_softmax), log_min_p <= 0; the unconditional rows must be finite.  Neither row
 * start nor ld needs any alignment beyond 4 bytes (16-byte accesses are used where a row allows them), and the values do not
 * depend on it: the order of every sum is a function of the element index alone, so equal rows give equal bits wherever they lie.
 * mg_guidance_follow: the negative half of a guided batch follows the guided half after the bookkeeping launch:
 *   token[R + r] = token[r];  d_pos[R + r] += delta  (pos_stride 1; d_pos NULL or pos_stride 0: positions left alone), r < R.  */
int mg_logits_guidance_f32(float* cond, int64_t ld_cond, const float* uncond, int64_t ld_uncond, int32_t R, int32_t V, float scale,
                           float log_min_p, void* stream);
int mg_guidance_follow(int64_t* token, int32_t* d_pos, int32_t R, int32_t delta, int32_t pos_stride, void* stream);

/* Token log-probabilities (ABI 16; DESIGN.md "Token log-probabilities"; host statement: magma_amd/sampling.py, token_logprobs):
 * how probable the model found a token, and the n_top most probable tokens beside it, in ONE enqueue-only, graph-capturable
 * launch of one workgroup per row; no allocation, no scratch.  logits [R, ld] fp32 (columns >= V are not read), token [R] int64.
 * Per row r, with column c = state[0] (device int32, read at run time: the step of a generate() loop) or c = 0 when state is NULL:
 *   lp[r * ld_lp + c] = (x[t] - m) - log sum_v exp(x[v] - m), t = token[r], m the row maximum -- the arithmetic and the reduction
 *     tree of mg_beam_topk_f32 (the same device code);
 *   top_id / top_lp [(r * cols + c) * n_top + j], j < n_top: the n_top most probable tokens of the row, ranked by RAW LOGIT
 *     descending, lower token id first -- reproducible from the logits alone, monotone in the log-probability, and entry 0 is what
 *     mg_argmax_f32 selects -- each value formed by the expression of lp.
 * n_top in [0, 20] and <= V (anything else is refused before the launch); n_top = 0 takes NULL top pointers and runs no selection
 * pass.  c outside [0, cols) writes nothing; a token outside [0, V) gives lp = -inf and reads nothing, the lists are still written.
 * Needs 1 <= cols <= ld_lp.                                                                                                   */
#define MG_LOGPROBS_MAX_TOP 20
int mg_token_logprobs_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const int64_t* token, const int32_t* state,
                          float* lp, int64_t ld_lp, int32_t cols, int32_t n_top, int32_t* top_id, float* top_lp, void* stream);

/* The same with a row indirection (ABI 19; DESIGN.md "Ranking choices"): N entries, one workgroup each; entry i gives
 *   lp[i] = (x[t] - m) - log sum_v exp(x[v] - m), x = logits row row_of[i] (logits [n_rows, ld] fp32), t = token[i],
 * by mg_token_logprobs_f32's device body in its n_top = 0 form -- the same bits for the same row and token -- so the edges out of
 * one trie node share their parent's row without a copy.  row_of / token [N] int32.  A row outside [0, n_rows) or a token outside
 * [0, V) reads nothing and gives -inf.                                                                                       */
int mg_token_logprobs_rows_f32(const float* logits, int64_t ld, int32_t n_rows, int32_t V, const int32_t* row_of,
                               const int32_t* token, int32_t N, float* lp, void* stream);

/* Contrastive search (ABI 22; Su et al. 2022, "A Contrastive Framework for Neural Text Generation"; DESIGN.md "Contrastive
 * search"; host statement: magma_amd/sampling.py, contrastive_rank / contrastive_search).  A sample owns a group of k <= 16 cache
 * rows b*k .. b*k + k - 1, one per candidate token; four enqueue-only, graph-capturable launches follow the head of a token step
 * over those R = B * k rows (no allocation, no scratch, no host round trip, nothing shared between workgroups of a launch):
 *
 * mg_contrastive_topk_f32: per sample b the k most probable tokens of logits row src[b] (logits [R, ld] fp32, columns >= V are not
 *   read; src [B] int32, a value outside the sample's group reads row b*k), ranked by raw logit descending, lower id first -- the
 *   device body of mg_token_logprobs_f32 -- as int64 into token[b*k + j] (the next step's input ids) and
 *   cand_p[b*k + j] = exp((x - max) - logsumexp), the fp32 softmax probability.
 * mg_contrastive_sim_bf16: hidden [R, ld_hidden] bf16 (the candidates' ln_f outputs), the context store ctx [B, Tmax, d] bf16 and
 *   ctx_len [B] int32 (device; clamped to [0, Tmax]) -> part [B, n_chunk, k] fp32, n_chunk = ceil(Tmax / MG_CONTRASTIVE_CHUNK):
 *   part[b, c, j] = max over the valid positions t of chunk c of  <h_j, c_t> / (|h_j| |c_t|)  in fp32 from the bf16 values (norms
 *   from the same values; a zero vector gives 0), or -1e30 for a chunk without a valid position.  Grid (n_chunk, B).  d must be a
 *   multiple of 256, ld_hidden >= d a multiple of 8, hidden and ctx 16-byte aligned.  len_max: the caller's host-side upper bound of
 *   ctx_len's entries, refused when it exceeds Tmax.
 * mg_contrastive_finish: one workgroup.  Per sample: penalty_j = max over the chunks of part (0 without any context position),
 *   score_j = (1 - alpha) * cand_p[b*k + j] - alpha * penalty_j in fp32, j* = the first largest.  Writes token[b*k + j*] into
 *   history[(b*k + j) * ld_history + step] for every j < k (step = state[0]; nothing outside [0, history_cols)), src[b] = b*k + j*,
 *   hidden row b*k + j* into ctx[b, ctx_len[b]] and ctx_len[b] += 1 (both only while ctx_len[b] < Tmax); then mg_sample_finish's
 *   bookkeeping: state[1] = step if every sample's token is eos and state[1] < 0, state[0] = step + 1, d_pos[i] += delta for the
 *   R rows (pos_stride 1) or d_pos[0] (pos_stride 0; d_pos NULL: no advance).  alpha in (0, 1]; len_max as above, refused when
 *   len_max >= Tmax (no room to append).
 * mg_kv_broadcast_bf16: caches [L, R, H, Smax, 256] bf16.  For every row r of a group whose src[b] != r: the 256-element K and V
 *   rows of every layer and head at position d_pos[r * pos_stride] + pos_delta are copied from row src[b] (pos_delta = -1 behind
 *   mg_contrastive_finish, which has advanced the positions).  A src outside the group or a position outside [0, Smax) copies
 *   nothing; k = 1 launches nothing.  Not mg_kv_reorder_bf16: one position, not whole rows. */
#define MG_CONTRASTIVE_CHUNK 32
#define MG_CONTRASTIVE_MAX_K 16
int mg_contrastive_topk_f32(const float* logits, int64_t ld, int32_t R, int32_t V, const int32_t* src, int32_t B, int32_t k,
                            int64_t* token, float* cand_p, void* stream);
int mg_contrastive_sim_bf16(const mg_bf16* hidden, int64_t ld_hidden, const mg_bf16* ctx, int32_t B, int32_t Tmax, int32_t d,
                            const int32_t* ctx_len, int32_t len_max, int32_t k, float* part, int32_t n_chunk, void* stream);
int mg_contrastive_finish(const float* part, int32_t n_chunk, const float* cand_p, int32_t B, int32_t k, float alpha,
                          const mg_bf16* hidden, int64_t ld_hidden, int32_t d, mg_bf16* ctx, int32_t Tmax, int32_t* ctx_len,
                          int32_t len_max, int32_t* src, const int64_t* token, int64_t* history, int64_t ld_history,
                          int32_t history_cols, int64_t eos, int32_t* state, int32_t* d_pos, int32_t delta, int32_t pos_stride,
                          void* stream);
int mg_kv_broadcast_bf16(mg_bf16* kcache, mg_bf16* vcache, int32_t L, int32_t R, int32_t H, int32_t Smax, int32_t k,
                         const int32_t* src, const int32_t* d_pos, int32_t pos_stride, int32_t pos_delta, void* stream);

/* CLIP VisionTransformer front end and attention (encoder_name "clip" = ViT-B/32; reference magma/image_encoders.py:56-63):
 *   patchify   img [B,3,H,W] bf16 NCHW -> rows [B*(H/P)*(W/P), 3*P*P] in (c, py, px) order = the im2col of the stride-P patch
 *              conv, which then is mg_gemm_bf16 against conv1.weight.reshape(width, 3*P*P);
 *   vit_embed  out[b,0,:] = class_embedding + pos[0];  out[b,1+g,:] = patches[b*G+g,:] + pos[1+g]   (fp32 add, bf16 out);
 *   attn_small non-causal multi-head attention for short sequences (S <= 256, head dim 64): qkv [B*S, 3*H*64] = [q | k | v]
 *              with the in_proj bias already added, out [B*S, H*64]; fp32 scores / softmax, scale 1/8.              */
int mg_patchify_bf16(const mg_bf16* img, mg_bf16* out, int32_t B, int32_t H, int32_t W, int32_t P, void* stream);
int mg_vit_embed_bf16(const mg_bf16* patches, const mg_bf16* class_embedding, const mg_bf16* pos, mg_bf16* out, int32_t B,
                      int32_t G, int32_t width, void* stream);
int mg_attn_small_bf16(const mg_bf16* qkv, mg_bf16* out, int32_t B, int32_t S, int32_t H, void* stream);
/* Backward of mg_attn_small_bf16 (training the CLIP ViT encoder; autograd through nn.MultiheadAttention in the reference's
 * CLIP dependency): qkv [B*S, 3*H*64] as in the forward, d_out [B*S, H*64] -> d_qkv [B*S, 3*H*64].  Recomputes the
 * probabilities (fp32) per (b, h); S <= 64.                                                                         */
int mg_attn_small_bwd_bf16(const mg_bf16* qkv, const mg_bf16* d_out, mg_bf16* d_qkv, int32_t B, int32_t S, int32_t H, void* stream);

/* K4: 2x2 average pool, NHWC bf16.  x [B,H,W,C] -> y [B,H/2,W/2,C]  (stem pool and the anti-aliased stride of
 * CLIP's ModifiedResNet bottlenecks; trunk selected at reference magma/image_encoders.py:65-74).              */
int mg_avgpool2_nhwc_bf16(const mg_bf16* x, mg_bf16* y, int32_t B, int32_t H, int32_t W, int32_t C,
                          void* stream);

/* K1 stem conv1 of the same trunk (3->C, 3x3, stride 2, pad 1): explicit im2col of the NCHW
 * bf16 image into [B*(H/2)*(W/2), 32] (27 taps*channels + 5 zero columns,
 * column = c*9 + ky*3 + kx, i.e. the conv weight's own
 * [cout, 3, 3, 3] flattening) for mg_gemm_bf16.                                */
int mg_stem_im2col_bf16(const mg_bf16* img_nchw, mg_bf16* out, int32_t B, int32_t H, int32_t W,
                        void* stream);

/* NF-ResNet-50 image encoder (encoder_name "nfresnet50"; reference magma/image_encoders.py:31-45 = timm nf_resnet50 minus its
 * classifier + AdaptiveAvgPool2d((1,1)), feeding the pooled ImagePrefix branch magma/image_prefix.py:17,67-72,96-101).  The
 * convolutions are mg_gemm_bf16; these are the pieces around them (csrc/nfnet.hip):
 *   weight_standardize  timm ScaledStdConv2d's weight transform: out[o, :] = (w[o, :] - mean_o) * rsqrt(var_o + eps) * gain[o] * scale
 *                       (biased variance over the cin*kh*kw fan-in; scale = gamma * fan_in^-0.5 from the caller), w [cout, cin, kh, kw]
 *                       bf16 -> out [cout, ldo] bf16 zero padded; to_khwc = 1 permutes the columns to (ky, kx, cin), the order of the
 *                       implicit-im2col 3x3 A loader (MG_A_CONV3X3), 0 keeps (cin, ky, kx) (1x1 convs, mg_im2col_nchw_bf16).
 *   im2col_nchw         img [B, C, H, W] bf16 -> rows [B*Ho*Wo, ldo], column (c*k + ky)*k + kx, zero padded (the 7x7 / stride-2 stem).
 *   maxpool3x3s2        MaxPool2d(3, stride 2, padding 1) on NHWC: x [B,H,W,C] -> y [B,(H-1)/2+1,(W-1)/2+1,C].
 *   subsample2          y[b,i,j,:] = x[b,2i,2j,:] (a stride-2, padding-1 3x3 conv = its stride-1 output at the even positions).
 *   relu_mean_rows      y[b, c] = mean_p relu(x[b, p, c]), x [B, HW, C]: final_act + AdaptiveAvgPool2d((1,1)).                          */
int mg_weight_standardize_bf16(const mg_bf16* w, const mg_bf16* gain, mg_bf16* out, int32_t cout, int32_t cin, int32_t kh,
                               int32_t kw, int64_t ldo, int32_t to_khwc, float scale, float eps, void* stream);
int mg_im2col_nchw_bf16(const mg_bf16* img, mg_bf16* out, int32_t B, int32_t C, int32_t H, int32_t W, int32_t k, int32_t stride,
                        int32_t pad, int32_t ldo, void* stream);
int mg_maxpool3x3s2_nhwc_bf16(const mg_bf16* x, mg_bf16* y, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int mg_subsample2_nhwc_bf16(const mg_bf16* x, mg_bf16* y, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int mg_relu_mean_rows_bf16(const mg_bf16* x, mg_bf16* y, int32_t B, int32_t HW, int32_t C, void* stream);
/* ... and their backward forms (training the nfresnet50 encoder, reference default freeze_img_encoder: false):
 *   weight_standardize_bwd  dwhat [cout, ldd] fp32 = gradient wrt the standardised weights in the weight's own (cin,ky,kx) order;
 *                           dw [cout, fan_in] += r (dn - mean(dn) - n mean(dn n)), dgain [cout] += scale sum(dwhat n),
 *                           n = (w - mean) r, r = rsqrt(var + eps), dn = dwhat * gain * scale   (fp32 accumulate into the caller's buffers);
 *   maxpool3x3s2_bwd        dx [B,H,W,C] from dy [B,Ho,Wo,C]: routed to the first maximum of each window (PyTorch's choice), as a gather;
 *   subsample2_bwd          dx[b,2i,2j,:] = dy[b,i,j,:], zero elsewhere;
 *   relu_mean_rows_bwd      dx[b,p,c] = x[b,p,c] > 0 ? g[b,c] / HW : 0.                                                                   */
int mg_weight_standardize_bwd_f32(const mg_bf16* w, const mg_bf16* gain, const float* dwhat, int64_t ldd, float* dw, float* dgain,
                                  int32_t cout, int32_t fan_in, float scale, float eps, float dmult /* dwhat is read times dmult */, void* stream);
int mg_maxpool3x3s2_bwd_nhwc_bf16(const mg_bf16* x, const mg_bf16* dy, mg_bf16* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int mg_subsample2_bwd_nhwc_bf16(const mg_bf16* dy, mg_bf16* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int mg_relu_mean_rows_bwd_bf16(const mg_bf16* x, const mg_bf16* g, mg_bf16* dx, int32_t B, int32_t HW, int32_t C, void* stream);

/* Data-parallel exchange step over RCCL / xGMI (csrc/comm.hip): the seam that replaces DeepSpeed's gradient reduction
 * (reference magma/train_loop.py:18-19 model_engine.backward / .step, train.py:103-111 deepspeed.initialize, magma/utils.py:26-34
 * reduce_losses).  One communicator per process (= per GPU; mg_comm_init binds the CURRENT HIP device):
 *   mg_comm_unique_id   rank 0 draws the 128-byte id, the caller hands it to every rank over any side channel;
 *   mg_comm_init        collective over all ranks; *comm_out = opaque handle;
 *   mg_comm_allreduce_sum  in-place SUM over the ranks, count elements of dtype MG_COMM_F32 / MG_COMM_BF16, enqueued on
 *                       `stream` (the mean of the reference's ZeRO-2 reduction is the 1/world folded into mg_adamw_*);
 *   mg_comm_broadcast   in-place from `root` (whole-model broadcast at engine construction; MG_COMM_BYTES = raw bytes);
 *   mg_comm_destroy.
 * RCCL is loaded with dlopen at the first call (the copy already in the process if there is one): MG_ERR_COMM if absent. */
#define MG_COMM_F32 0
#define MG_COMM_BF16 1
#define MG_COMM_BYTES 2
int mg_comm_unique_id(uint8_t* id128);
int mg_comm_init(void** comm_out, const uint8_t* id128, int32_t rank, int32_t world);
int mg_comm_allreduce_sum(void* comm, void* buf, int64_t count, int32_t dtype, void* stream);
int mg_comm_broadcast(void* comm, void* buf, int64_t count, int32_t dtype, int32_t root, void* stream);
int mg_comm_destroy(void* comm);

/* K20 (integer, exact): reference magma/utils.py:334-364 build_labels.
 * labels[b, :P] = -100; labels[b, P+t] = captions[b, t] up to and including
 * the first eos of the row; -100 after.  captions/labels [B, S] int64.       */
int mg_build_labels_i64(const int64_t* captions, int64_t* labels, int32_t B, int32_t S, int32_t P,
                        int64_t eos, void* stream);

/* K19: shifted cross-entropy of the LM call with labels (reference magma/magma.py:270-274; loss computed inside
 * the fork's GPTNeoForCausalLM.forward in fp32).  For each row r of `logits` [R, V] fp32 with target
 * tgt[r] (int64; -100, or any other value outside [0, V) = ignore): loss_row[r] = logsumexp - logit[tgt] (0 if
 * ignored).  The caller passes already-shifted rows.  mg_ce_reduce produces
 * mean over valid rows (targets in [0, V)) into out[0] and the valid count into out[1].          */
int mg_ce_rows_f32(const float* logits, int64_t ld, const int64_t* tgt, float* loss_row,
                   int32_t R, int32_t V, void* stream);
int mg_ce_reduce_f32(const float* loss_row, const int64_t* tgt, int32_t R, int32_t V, float* out,
                     void* stream);

/* ===================== training path (backward + optimizer) =====================
 * Replaces model_engine.backward(loss) / model_engine.step() of reference magma/train_loop.py:15-19 (torch.autograd +
 * the DeepSpeed engine configured at magma/config.py:113-134).                                                  */

/* out[C,R] = in[R,C]^T (batched).  Feeds the wgrad GEMMs, which contract over the
 * row index M of activations: dW[N,K] = dY^T[N,M] * (X^T[K,M])^T.
 * C % 8 == 0; R is any positive count with ld_out >= round_up(R, 8): the columns [R, round_up(R, 8)) of out are written as zeros
 * (the K padding of that GEMM), nothing beyond them is touched.                     */
int mg_transpose_bf16(const mg_bf16* in, int64_t ld_in, int64_t bs_in, mg_bf16* out, int64_t ld_out,
                      int64_t bs_out, int32_t R, int32_t C, int32_t batch, void* stream);
/* The same transpose of ONE matrix that also accumulates colsum[c] += sum_r in[r][c] (fp32): the bias gradient and the weight-gradient
 * operand of a Linear (reference adapters.py:18-25 Linear layers; torch.autograd in the reference) from one pass over its output gradient. */
int mg_transpose_colsum_bf16(const mg_bf16* in, int64_t ld_in, mg_bf16* out, int64_t ld_out, int32_t R, int32_t C,
                             float* colsum, void* stream);

/* per-head transposes for the attention kernels, column-tiled: dst[(((b*H+h)*(ld/32) + s/32)*256 + d)*32 + s%32]
 * = src[b*sb + s*ss + h*sh + d]; ld = round_up(S,32), zero filled.                                              */
int mg_head_transpose_bf16(const mg_bf16* src, int64_t sb, int64_t ss, int64_t sh, mg_bf16* dst, int32_t ld,
                           int32_t B, int32_t H, int32_t S, void* stream);

/* out[n] += sum_m x[m][n] * (y ? y[m][n] : 1)  (bias / affine gradients, fp32 atomics). */
int mg_colsum_f32(const mg_bf16* x, int64_t ldx, const mg_bf16* y, int64_t ldy, float* out, int32_t M,
                  int32_t N, void* stream);

/* The same sums without atomics: one partial per 256 rows goes to `parts` (fp32 [mg_colsum_det_parts(M), N], contents
 * ignored on entry) and a second launch adds the partials to out in row order, so the result is the same bits in every run.
 * For sums that feed a rounding decision (the batch-statistics BatchNorm). */
int64_t mg_colsum_det_parts(int32_t M);
int mg_colsum_det_f32(const mg_bf16* x, int64_t ldx, const mg_bf16* y, int64_t ldy, float* out, float* parts, int32_t M,
                      int32_t N, void* stream);

/* LayerNorm input gradient (+ optional residual add, optional xhat output).         */
int mg_layernorm_bwd_bf16(const mg_bf16* dy, int64_t lddy, const mg_bf16* x, int64_t ldx, const float* gamma,
                          const mg_bf16* res, int64_t ldr, mg_bf16* dx, int64_t lddx, mg_bf16* xhat,
                          int64_t ldxh, int32_t rows, int32_t d, float eps, void* stream);

/* dlogits = (softmax(logits) - onehot(tgt)) / n_valid, bf16, zero padded to ldo.
 * stats = output of mg_ce_reduce_f32 (stats[1] = number of valid targets).          */
int mg_ce_bwd_bf16(const float* logits, int64_t ld, const int64_t* tgt, const float* stats, mg_bf16* out,
                   int64_t ldo, int32_t R, int32_t V, void* stream);

/* inverse rotary on dq,dk and merge dq|dk|dv [B,H,S,256] -> dqkv [B*S, 3*H*256].    */
int mg_rotary_merge_bwd_bf16(const mg_bf16* dq, const mg_bf16* dk, const mg_bf16* dv, int32_t B, int32_t S,
                             int32_t H, int32_t rot_dim, const float* sin_t, const float* cos_t,
                             mg_bf16* dqkv, void* stream);

/* causal flash-attention backward, head dim 256 (recomputes P from q,k,lse).
 * q,k,v [B,H,S,256]; qt,kt,dOt [B,H,ld_t/32,256,32] (column-tiled transposes from mg_head_transpose_bf16,
 * ld_t = round_up(S,32), zero padded);
 * dO [B*S,H*256]; O [B*S, >= H*256] with row stride ld_o elements (ABI 2: the attention output may sit in a wider
 * [ctx | t] buffer, the operand of the [W_out | W_up] GEMM); lse [B,H,S]; D = fp32 workspace of 2*B*H*S floats ({-16 lse, -rowsum(dO o O)}
 * per query, written by the first launch).                                           */
int mg_attn_bwd_bf16(const mg_bf16* q, const mg_bf16* k, const mg_bf16* v, const mg_bf16* qt,
                     const mg_bf16* kt, const mg_bf16* dO, const mg_bf16* dOt, const mg_bf16* O,
                     const float* lse, float* D, mg_bf16* dq, mg_bf16* dk, mg_bf16* dv, int32_t B,
                     int32_t H, int32_t S, int32_t ld_t, int64_t ld_o, void* stream);

/* The same backward written straight into the gradient of the fused qkv projection (autograd through
 * GPTJAttention's rotary + head split, /root/reference call site magma/magma.py:263-276 -> HF modeling_gptj):
 * dqkv [B*S, 3*H*256] = [dq | dk | dv] per token, the inverse GPT-J rotary R(-theta_s) applied to the first
 * rot_dim columns of every dq and dk head (sin_t, cos_t fp32 [>= S, rot_dim/2]).  Equals mg_attn_bwd_bf16
 * followed by mg_rotary_merge_bwd_bf16 with one bf16 rounding instead of two.  dOt is a WORKSPACE
 * [B,H,ld_t/32,256,32] here: the first launch transposes dO into it while it computes D.               */
int mg_attn_bwd_merged_bf16(const mg_bf16* q, const mg_bf16* k, const mg_bf16* v, const mg_bf16* qt,
                            const mg_bf16* kt, const mg_bf16* dO, mg_bf16* dOt, const mg_bf16* O,
                            const float* lse, float* D, mg_bf16* dqkv, int32_t rot_dim, const float* sin_t,
                            const float* cos_t, int32_t B, int32_t H, int32_t S, int32_t ld_t, int64_t ld_o, void* stream);

/* ---- attention without transposed operand images (round 6, csrc/attention_tr.hip) -------------------------------------------------
 * The path replaced: reference magma/magma.py:263-276 -> HF GPTJAttention (rotary on q / k, causal softmax(q k^T / 16) v) and its
 * autograd.  The s-contraction operands (V^T in the forward; Q^T, dO^T, K^T in the backward) are read from the ROW images in LDS with
 * ds_read_b64_tr_b16, so no transposed tensor exists in HBM, and q / k / v are taken as rows of 256 at arbitrary strides:
 * position s of head (b, h) at  ptr + b stride_b + h stride_h + s ld_row  (elements; ld_row >= 256, all multiples of 8,
 * S ld_row 2 < 2^31).  [B,H,S,256]: ld_row 256, stride_h S 256, stride_b H S 256.  The fused qkv activation [B*S, 3 H 256] ITSELF:
 * q = qkv, k = qkv + H 256, v = qkv + 2 H 256, ld_row 3 H 256, stride_h 256, stride_b S 3 H 256 -- after mg_rotary_qk_inplace_bf16
 * there is no split pass and no copy of q, k or v.                                                                                   */
/* GPT-J rotary (interleaved pairs) applied in place to the first rot_dim columns of every q and k head of qkv [B*S, ld_qkv >= 3 H 256],
 * angles of position s = row % S (tables sin_t / cos_t fp32 [>= S, rot_dim / 2]); v is not touched.                                  */
int mg_rotary_qk_inplace_bf16(mg_bf16* qkv, int64_t ld_qkv, int32_t B, int32_t S, int32_t H, int32_t rot_dim,
                              const float* sin_t, const float* cos_t, void* stream);
/* causal flash-attention forward: out [B*S, >= H*256] bf16 at row stride ld_out (0 = H*256; % 8 == 0), lse [B,H,S] fp32 or NULL.
 * Same arithmetic as mg_attn_prefill_bf16 (fp32 online softmax, 1/16 scale).                                                          */
int mg_attn_fwd_rows_bf16(const mg_bf16* q, const mg_bf16* k, const mg_bf16* v, int64_t ld_row, int64_t stride_b,
                          int64_t stride_h, mg_bf16* out, int64_t ld_out, float* lse, int32_t B, int32_t H, int32_t S, void* stream);
/* backward: dO [B*S, H*256]; O [B*S, >= H*256] at row stride ld_o; lse [B,H,S]; D fp32 workspace of 2 B H S floats.  Output EITHER
 * dq, dk, dv [B,H,S,256] (dqkv NULL) OR dqkv [B*S, 3 H 256] = the gradient of the fused qkv projection with the inverse rotary applied
 * to the first rot_dim columns of every dq and dk head (dq, dk, dv NULL) -- as mg_attn_bwd_bf16 / mg_attn_bwd_merged_bf16.
 * dqkv8 / dqkv8_scales (or NULL): also the OCP MX e4m3 copy of dqkv, [B*S, 3 H 256] bytes + E8M0 scales of mg_mx_scale_bytes(B*S, 3 H 256)
 * bytes, bit for bit what mg_quantize_mx_fp8 makes of the bf16 dqkv -- the operand of the qkv dgrad's mg_gemm_mx_fp8 (BASELINE config[4]),
 * written from the epilogue's row pieces; dqkv itself may then be NULL (no bf16 copy).                                               */
int mg_attn_bwd_rows_bf16(const mg_bf16* q, const mg_bf16* k, const mg_bf16* v, int64_t ld_row, int64_t stride_b,
                          int64_t stride_h, const mg_bf16* dO, const mg_bf16* O, int64_t ld_o, const float* lse, float* D,
                          mg_bf16* dq, mg_bf16* dk, mg_bf16* dv, mg_bf16* dqkv, int32_t rot_dim, const float* sin_t,
                          const float* cos_t, int32_t B, int32_t H, int32_t S, uint8_t* dqkv8, uint8_t* dqkv8_scales, int32_t first_rows, void* stream);

/* CLIP trunk backward helpers */
int mg_avgpool2_bwd_nhwc_bf16(const mg_bf16* dy, const mg_bf16* gate, mg_bf16* dx, int32_t B, int32_t H, int32_t W, int32_t C, void* stream);
int mg_mul_bf16(const mg_bf16* a, const mg_bf16* b, mg_bf16* out, int64_t n, void* stream);
/* torch.nn.GELU() (erf form) for adapters built with activation=nn.GELU (reference magma/adapters.py:11,20): y = gelu(x) when g is NULL,
 * y = g * gelu'(x) otherwise, over [rows, cols] bf16 with row strides (elements; cols % 8 == 0); in place allowed.  A pass of its own:
 * the erf polynomial is kept out of the GEMM epilogues (it cost the 256x256 kernels registers).                                      */
int mg_gelu_erf_bf16(const mg_bf16* x, int64_t ldx, const mg_bf16* g, int64_t ldg, mg_bf16* y, int64_t ldy, int32_t rows,
                     int32_t cols, void* stream);
int mg_scale_rows_acc_f32(float* dst, const float* src, int64_t ld_src, const float* row_scale, int32_t rows,
                          int32_t cols, void* stream);
/* The parameter gradients of a conv + frozen-statistics BatchNorm unit from the UNSCALED fp32 product src = g^T a ([rows = Cout,
 * cols = Cin k k], row stride ld_src), the bf16 weight w [rows, cols] and gsum[r] = sum_m g[m][r] (ABI 27):
 *   dst[r][c] += src[r][c] * row_scale[r];   dbeta[r] += gsum[r];
 *   dgamma[r] += rsqrt(var[r] + eps) * (sum_c src[r][c] * w[r][c] - mean[r] * gsum[r])
 * sum_c src w = sum_m g z with z = a W^T, the raw convolution output that the forward folds away: dgamma is the layer's own
 * sum_m g (z - mean) rstd for every gamma, zero included.  mg_bn_param_grad_f32 / mg_transpose_bn_param_grad_bf16 below recover the
 * normalised activation from the rounded bf16 output instead, (y - sub - beta) / gamma: 2^-9 |y| / |gamma| off per element, and 0 at gamma == 0. */
int mg_scale_rows_acc_bn_grad_f32(float* dst, const float* src, int64_t ld_src, const mg_bf16* w, const float* row_scale,
                                  const float* mean, const float* var, float eps, const float* gsum, float* dgamma, float* dbeta,
                                  int32_t rows, int32_t cols, void* stream);
int mg_add_gate_bf16(const mg_bf16* a, const mg_bf16* b, const mg_bf16* gate, mg_bf16* out, int64_t n, void* stream);
int mg_bn_param_grad_f32(const mg_bf16* g, const mg_bf16* y, const mg_bf16* sub, const float* gamma,
                         const float* beta, float* dgamma, float* dbeta, int32_t M, int32_t C, void* stream);
/* The same sums taken while g is transposed for the convolution's weight-gradient GEMM (out = g^T [C, ld_out], as mg_transpose_bf16;
 * y / sub in g's layout): one pass over g instead of two, from a grid of 64x64 tiles (ABI 6).                                   */
int mg_transpose_bn_param_grad_bf16(const mg_bf16* g, int64_t ld_in, mg_bf16* out, int64_t ld_out, int32_t R, int32_t C,
                                    const mg_bf16* y, const mg_bf16* sub, const float* gamma, const float* beta,
                                    float* dgamma, float* dbeta, void* stream);
/* trainable conv weight [Cout][Cin][k][k] (k = 1, 3) -> row-major GEMM operand, rows zero padded to ldo:
 *   mode 0: out[co][tap*Cin + ci] = w[co][ci][ky][kx]                       (forward, implicit-im2col order)
 *   mode 1: out[ci][tap*Cout + co] = bf16(w[co][ci][k-1-ky][k-1-kx] * scale[co])   (dgrad: flipped taps, BN scale folded)
 * (one launch instead of PyTorch's permute / flip / multiply / cast / pad copies, every step, for each of the 127 convs). */
int mg_conv_weight_relayout_bf16(const mg_bf16* w, const float* scale, mg_bf16* out, int64_t ldo, int32_t Cout, int32_t Cin,
                                 int32_t k, int32_t mode, void* stream);
/* frozen-statistics BatchNorm as a per-channel affine for the conv epilogues (one launch per BN and step):
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale; all fp32 [C].                                   */
int mg_bn_fold_f32(const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                   float* scale, float* shift, int32_t C, void* stream);
/* The two calls above for MANY convolutions / BatchNorms in one launch each (ABI 6): the training engine re-derives the GEMM
 * operands of all 127 trunk convolutions (forward + dgrad layout) and the folded affine of their BatchNorms once per step --
 * 2 launches instead of ~380.  `jobs`: DEVICE array (caller-owned, 8-byte aligned), sorted by first_block; job i covers the
 * workgroups [first_block, first_block + ceil(rows * ldo / 256)) resp. [first_block, first_block + ceil(C / 256));
 * total_blocks = the end of the last job.  Same arithmetic, element for element, as the single-job entry points.
 * (reference: the convolutions / BatchNorms of magma/image_encoders.py:48-76's CLIP trunk, trained as in magma/magma.py:98-100) */
typedef struct mg_relayout_job {
  const mg_bf16* w;      /* [Cout][Cin][k][k] */
  const float* scale;    /* mode 1: [Cout] or NULL */
  mg_bf16* out;          /* rows x ldo */
  int64_t ldo;
  int32_t Cout, Cin, k, mode;
  int64_t first_block;
} mg_relayout_job;
typedef struct mg_bn_fold_job {
  const float* gamma; const float* beta; const float* mean; const float* var;
  float* scale; float* shift;
  float eps; int32_t C;
  int64_t first_block;
} mg_bn_fold_job;
int mg_conv_weight_relayout_batch(const mg_relayout_job* jobs, int32_t njobs, int64_t total_blocks, void* stream);
int mg_bn_fold_batch(const mg_bn_fold_job* jobs, int32_t njobs, int64_t total_blocks, void* stream);
int mg_im2col_t_bf16(const mg_bf16* x, mg_bf16* out, int64_t ldo, int32_t B, int32_t H, int32_t W, int32_t Cin, void* stream);

/* batch-statistics BatchNorm of the CLIP trunk in training (the reference's tower runs in train mode after its
 * first eval phase, reference train.py:164,182).  z = raw conv output [M, C] bf16 (M = B*H*W); sum / sumsq = per-channel sums
 * of z and z*z (mg_colsum_det_f32: reproducible, they feed bf16 roundings).  fold: scale = gamma * rstd, shift = beta - mean * scale, and running_mean / running_var
 * (may be NULL) updated like nn.BatchNorm2d (momentum, unbiased variance).  apply: y = [relu](z*scale + shift [+ res]).
 * bwd_dz: dz = gamma * rstd * (g - dbeta/M - xhat * dgamma/M) with xhat = (z - mean) * rstd, dgamma / dbeta = this call's
 * per-channel sums of g * xhat and g.                                                                                    */
int mg_bn_batch_fold_f32(const float* sum, const float* sumsq, const float* gamma, const float* beta, int64_t M, float eps,
                         float momentum, float* running_mean, float* running_var, float* scale, float* shift, float* mean,
                         float* rstd, int32_t C, void* stream);
int mg_bn_apply_bf16(const mg_bf16* z, const float* scale, const float* shift, const mg_bf16* res, int32_t relu, mg_bf16* y,
                     int64_t M, int32_t C, void* stream);
int mg_bn_bwd_dz_bf16(const mg_bf16* g, const mg_bf16* z, const float* mean, const float* rstd, const float* gamma,
                      const float* dgamma, const float* dbeta, mg_bf16* dz, int64_t M, int32_t C, void* stream);

/* optimizer (replaces DeepSpeed's fp16 ZeRO-2 step: global-norm clip + AdamW on fp32
 * master copies, reference train.py:96-101, config.py:124-134).                     */
int mg_sumsq_f32(const float* g, int64_t n, float* out, void* stream);
int mg_adamw_f32(float* p, float* m, float* v, const float* g, mg_bf16* p_bf16, int64_t n, float lr,
                 float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                 const float* norm_sq, float grad_scale, void* stream);
/* data-parallel exchange (reference train_loop.py:18-19 -> DeepSpeed ZeRO-2 reduces fp16 gradients; here bf16, 0.77 GB
 * per step for MAGMA_v1): the fp32 flat gradients are cast into bf16 buckets, summed over the ranks by RCCL
 * (torch.distributed, host side) and consumed as bf16 by the same fused clip + AdamW (g holds the SUM; grad_scale the
 * 1 / (gas * world) of the mean).  n % 4 == 0 for the cast.                                                          */
int mg_cast_f32_bf16(const float* src, mg_bf16* dst, int64_t n, void* stream);
int mg_sumsq_bf16(const mg_bf16* g, int64_t n, float* out, void* stream);
int mg_adamw_gbf16_f32(float* p, float* m, float* v, const mg_bf16* g, mg_bf16* p_bf16, int64_t n, float lr,
                       float beta1, float beta2, float eps, float weight_decay, int32_t step, float max_norm,
                       const float* norm_sq, float grad_scale, void* stream);

/* ---- fp8 attention forward (BASELINE config[4]: "fp8 MFMA path for GPT-J attention"; reference call site magma/magma.py:270-274) ----
 * mg_rotary_split_fp8: the training form of the rotary split (everything mg_rotary_split_train_bf16 writes except V^T: the backward
 * stays bf16) plus OCP MX e4m3 copies for the forward: q8 / k8 [B,H,S,256] with ONE power-of-two (E8M0) scale per token in
 * eq / ek [B,H,Sp] bytes, Sp = mg_attn_fp8_scale_stride(S); v8t [B,H,ceil(S/64),256,64] = V^T in 64-key tiles with one E8M0 per
 * (d, 32 keys) in sv8 [B,H,ceil(S/64),512] (layout [key block][d % 32][d / 32]); inside a tile the keys are stored in the order
 * the attention kernel's accumulators hold them (attention.hip: rotary_split_fp8_kernel).  qt / kt may be NULL (no backward);
 * q / k / v may be NULL together (forward only).
 * mg_attn_prefill_fp8: causal flash attention on v_mfma_scale_f32_32x32x64_f8f6f4 with those operands, fp32 softmax, P as
 * e4m3(16 p) with scale 2^-4; outputs as mg_attn_prefill_bf16 (out bf16 [B*S, >= H*256] at row stride ld_out % 8 == 0, lse fp32).
 * ABI 5: out8 / out8_scales (or NULL) = also the OCP MX e4m3 copy of out ([B*S, ld_out8 = ceil(H*256 / 128) * 128] bytes + E8M0 scales
 * of mg_mx_scale_bytes(B*S, H*256) bytes), bit for bit what mg_quantize_mx_fp8 makes of it: the operand of out_proj's MX GEMM.      */
int32_t mg_attn_fp8_scale_stride(int32_t S);
int mg_rotary_split_fp8(const mg_bf16* qkv, int32_t B, int32_t S, int32_t H, int32_t rot_dim, const float* sin_t,
                        const float* cos_t, mg_bf16* q, mg_bf16* k, mg_bf16* v, mg_bf16* qt, mg_bf16* kt, int32_t ld_t,
                        uint8_t* q8, uint8_t* k8, uint8_t* v8t, uint8_t* eq, uint8_t* ek, uint8_t* sv8, int32_t inplace, void* stream);
int mg_attn_prefill_fp8(const uint8_t* q8, const uint8_t* k8, const uint8_t* v8t, const uint8_t* eq, const uint8_t* ek,
                        const uint8_t* sv8, mg_bf16* out, int64_t ld_out, float* lse, int32_t B, int32_t H, int32_t S,
                        uint8_t* out8, int64_t ld_out8, uint8_t* out8_scales, void* stream);

/* A HIP stream whose kernels never run on `reserve` of the device's CUs (spread evenly; hipExtStreamCreateWithCUMask): the
 * training engine can run its compute on it so that the RCCL kernels of the gradient exchange (reference train_loop.py:18-19 /
 * DeepSpeed's overlapped reduce) always find free CUs instead of waiting for tile-GEMM workgroup boundaries.  Off by default
 * (MAGMA_DP_RESERVE_CUS).  The caller destroys the stream.                                                             */
int mg_stream_create_cu_mask(void** stream_out, int32_t reserve);
int mg_stream_destroy(void* stream);

/* ---- image preprocessing (reference magma/transforms.py:121-134) ----------------
 * One pass of Pillow's 8-bit antialiased resampling (ImagingResample, the arithmetic behind torchvision's
 * Resize(n, BICUBIC) on a PIL image): src is HWC uint8 RGB [H][W][3]; axis 1 resamples every row to
 * out_size pixels (dst [H][out_size][3]), axis 0 every column (dst [out_size][W][3]).  coeffs is
 * [out_size][ksize] int32 (22 fractional bits), bounds [out_size][2] = {first source index, count}; both
 * are built on the host exactly as Pillow's precompute_coeffs / normalize_coeffs_8bpc do.  Bit-exact.   */
int mg_resample_u8(const uint8_t* src, int32_t H, int32_t W, uint8_t* dst, int32_t out_size, int32_t axis,
                   const int32_t* coeffs, const int32_t* bounds, int32_t ksize, void* stream);
/* CenterCrop + ToTensor + Normalize: out[c][y][x] = (src[top+y][left+x][c] / 255 - mean[c]) / std[c] in
 * IEEE fp32 (CHW, n x n); mean3 / std3 are HOST pointers to 3 floats.                                   */
int mg_crop_normalize_f32(const uint8_t* src, int32_t H, int32_t W, int32_t top, int32_t left, int32_t n,
                          const float* mean3, const float* std3, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAGMA_HIP_H */
