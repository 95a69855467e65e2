/*
 * ovla.h -- C-ABI of libovla_hip.so: the MI355X (gfx950) kernels behind the OpenVLA-OFT
 * parallel-decoding action-chunk forward/backward path.
 *
 * The reference (ciccio42/openvla-oft) has NO native interface for this path: every FLOP is delegated to
 * PyTorch / timm / transformers / peft.  Each entry point below therefore cites the reference
 * *Python call site* whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch types.  All device buffers are caller-owned.
 *  - every op is `int ovla_<op>(const ovla_<op>_args*, void* hip_stream)`; returns 0 or a negative OVLA_E* code,
 *    `ovla_last_error()` returns a thread-local message.  Nothing is allocated, nothing synchronises the host;
 *    all kernels are stream-ordered on the given stream.
 *  - bf16 tensors are passed as `const void*` holding IEEE bfloat16 bit patterns; row-major; leading dimensions
 *    ("ld*") are in ELEMENTS.
 *  - "rows" of a token matrix are flattened (batch, position): row = b * S + s.
 */
#ifndef OVLA_H_
#define OVLA_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OVLA_OK 0
#define OVLA_EINVAL (-1)  /* malformed arguments (shape/alignment/null) */
#define OVLA_EARCH (-2)   /* device is not gfx950 */
#define OVLA_ELAUNCH (-3) /* HIP launch / runtime error */

#define OVLA_ABI_VERSION 1

const char* ovla_last_error(void);
int ovla_abi_version(void);
/* sha256 (first 32 hex digits) of the sources, headers and build script this library was compiled from (csrc/build.sh); the Python
 * loader compares it with the files next to the library and refuses a stale build. */
const char* ovla_build_hash(void);
/* Checks that `device` is a gfx950 part; returns OVLA_OK / OVLA_EARCH / OVLA_ELAUNCH. */
int ovla_check_device(int device);

/* ------------------------------------------------------------------------------------------------------------------
 * GEMM  C[M,N] = epilogue( A[M,K] . B[N,K]^T  (+ A2[M,K2] . B2[N,K2]^T) )          bf16 in, fp32 accumulate
 *
 * Replaces every nn.Linear on the path:
 *   Llama q/k/v/o/gate/up/down  (transformers LlamaDecoderLayer, call site prismatic/extern/hf/modeling_prismatic.py:632-643)
 *   timm Block qkv/proj/fc1/fc2 and patch_embed-as-GEMM (call site modeling_prismatic.py:201-227)
 *   PrismaticProjector fc1/fc2/fc3 (modeling_prismatic.py:250-262), ProprioProjector / NoisyActionProjector
 *   (prismatic/models/projectors.py:19-24,44-49), MLPResNet fc1 / block Linear (prismatic/models/action_heads.py:72-81),
 *   FiLM scale/shift (prismatic/models/film_vit_wrapper.py:65-67),
 * and, through the (A2,B2) "K-extension", peft's LoRA update  y += (alpha/r) * B(A x)  (vla-scripts/finetune.py:862-871):
 * A2 = scaled t = s * x A^T  [M, G*r],  B2 = stacked LoRA-B [N, r]; the column block of A2 used by an output tile is
 * (n0 / k2_group_n) * K2, so fused q|k|v and gate|up linears share one launch.
 * Because frozen weights are kept both as W [out,in] and W^T [in,out] in HBM, the same "NT" kernel computes the
 * backward data gradient dX = dY . W (A = dY, B = W^T).
 *
 * Epilogue order (each step rounds to bf16 like the reference's separate PyTorch ops do):
 *   v = alpha * acc;  v += bias[n];  [C_pre = v];  v = act(v);  v *= colscale[n];  v += residual[m,n];
 *   v = v * (1 + film_gamma[m / film_rows, n]) + film_beta[...]  ->  C
 * Backward epilogues (the data-gradient GEMM applies the producing activation's derivative instead of a separate pass):
 *   dact_mode 1: C[m,n] = v * act'(dact_src[m,n])               (dact_act: GELU / ReLU / SiLU / GELU-tanh; timm Mlp, projector)
 *   dact_mode 2: SwiGLU: g = dact_src[m,n], u = dact_src[m,n+N]; C[m,n] = v*u*silu'(g), C[m,n+N] = v*silu(g); C is [M,2N]
 *     (LlamaMLP down_proj(silu(gate) * up): the gradient of the fused gate|up pre-activations)
 * Requirements: K % 8 == 0, K2 % 8 == 0, N % 8 == 0, ld* % 8 == 0, 16-byte aligned base pointers.
 * split_k > 1 needs `workspace` of ovla_gemm_workspace_bytes() bytes.
 */
enum { OVLA_ACT_NONE = 0, OVLA_ACT_GELU = 1, OVLA_ACT_RELU = 2, OVLA_ACT_SILU = 3, OVLA_ACT_GELU_TANH = 4,
       /* ovla_gemm_bf16 only, on tiles 0 / 18 / 118 / 22 / 122 (the 4-wave configurations; tile 0 takes 18; K % 64 == 0): B = [gate; up] stacked ([N = 2 F, K], F % 128 == 0), C is [M, F] = bf16(bf16(silu(g)) * u) with g | u the
        * bf16-rounded projection outputs -- HF LlamaMLP's act_fn(gate_proj(x)) * up_proj(x) (modeling_llama.py) without the [M, 2 F] intermediate; nothing else
        * in the epilogue but alpha, the RMSNorm-fold row scale (rowscale_part; 22 / 122) and C_pre (the [M, 2 F] projection output, contiguous: row stride N; kept by training).
        * K-extension: 0 or 32 columns on 18 / 118, none on 22 / 122.  Same bits as ovla_gemm_bf16 + ovla_swiglu_fwd. */
       OVLA_ACT_SWIGLU = 5 };

typedef struct {
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  const void* A2; int64_t lda2;  /* optional K-extension (LoRA) */
  const void* B2; int64_t ldb2;
  void* C; int64_t ldc;          /* bf16 [M,N] */
  void* C_pre;                   /* optional bf16 [M,N] (ldc): value before the activation; with FiLM: before the modulation;
                                    with OVLA_ACT_SWIGLU: the [M, N = 2 F] projection output, CONTIGUOUS (row stride N, not ldc) */
  const void* bias;              /* optional bf16 [N] */
  const void* colscale;          /* optional bf16 [N]  (timm LayerScale) */
  const void* residual; int64_t ldr; /* optional bf16 [M,N] */
  const void* film_gamma;        /* optional bf16 [M/film_rows, N]  (FiLM) */
  const void* film_beta;
  int32_t film_rows;
  int32_t M, N, K, K2;
  int32_t k2_group_n;            /* 0: A2 column offset 0 for every tile */
  int32_t a_group_n;             /* >0: block-diagonal GEMM -- output columns [g*a_group_n, (g+1)*a_group_n) contract A columns
                                    [g*K, (g+1)*K) with B rows of the same column range (per-group LoRA dt = dy_g . B_g) */
  int32_t act;
  int32_t split_k;               /* <=1: none */
  int32_t tile;                  /* 0: auto; otherwise forces a tile configuration (tests / tuning): 1 (128x128), 2 (64x128), 5 (128x32),
                                    16 / 17 (256x256 on 4x2 / 2x4 waves), 18 (4-wave 256x256), 22 (4-wave 128x256); id + 100 = the same
                                    configuration with the hybrid schedule forced.  10 .. 15, 20, 21: the experimental BK = 32 ring kernel
                                    (plain epilogues and split-K only, no + 100 form).  6 (the skinny kernel) is what tile 0 resolves to for
                                    N = 32, K <= 3072, M >= 512 and takes no epilogue.  Any other id is OVLA_EINVAL ("unknown tile id"). */
  float alpha;                   /* scales the accumulator (LoRA alpha/r); 0 means 1 */
  const void* dact_src; int64_t ld_dact;   /* optional saved pre-activations for the backward epilogues above */
  int32_t dact_mode, dact_act;
  const void* rope_cos; const void* rope_sin;  /* optional bf16 [>= rope_S, 64] tables: RoPE (head_dim 128, HF rotate_half, position = */
  int32_t rope_S, rope_cols;                   /* row % rope_S) applied to output columns [0, rope_cols) -- the q | k heads of a fused
                                                  q|k|v projection (modeling_llama apply_rotary_pos_emb).  Excludes the other epilogues;
                                                  fused into the epilogue on tiles 1, 16, 17, 18 and 22 (and their + 100 forms) where the
                                                  shape allows, otherwise one extra ovla_rope launch: the same bits either way. */
  /* RMSNorm folded around the GEMM (the decoder's input_layernorm / post_attention_layernorm, HF LlamaRMSNorm at modeling_prismatic.py:632-643,
   * on the merged inference path; the norm WEIGHT is folded into B offline, B' = bf16(B * w[k])):
   *   producer side  rowsq_out [M, N/64] fp32: sum of squares of every 64-column group of the bf16 OUTPUT row (plain stores, one writer per
   *                  slot: summed later in slot order -- deterministic);
   *   consumer side  rowscale_part [M, rowscale_slots] fp32 = the producer's rowsq_out for this GEMM's A operand (rowscale_slots * 64 = K):
   *                  C = epilogue(acc * (alpha * rstd[m])), rstd[m] = rsqrt(sum(slots) / K + rowscale_eps): ONE fp32 factor alpha * rstd[m],
   *                  multiplied into the accumulator once -- the same bits whichever path a tile takes (interior, edge, K-split remainder);
   *                  rowscale_r [M] fp32 scratch receives rstd (the hybrid-remainder reduce reads it).
   * Both sides run on tiles 1 / 101 (128x128, what the batch-1 shapes M <= ~1k resolve to) and 22 / 122 (the 4-wave 128x256 configuration,
   * what the engine's batch-1 path forces; consumer side for K <= 4096, no producer side in a launch that fuses RoPE); any other schedule is an error. */
  float* rowsq_out;
  const float* rowscale_part; int32_t rowscale_slots; float rowscale_eps; float* rowscale_r;
  /* In-launch reduce of the hybrid schedule's K-split remainder tiles: device array of n_hybrid_counters uint32, ALL ZERO on entry (the kernel
   * leaves it all zero).  The last of a tile's K-part workgroups to arrive sums the slabs in slab order and runs the epilogue, so no separate
   * reduce launch is needed; same bits either way.  NULL / too few counters: a gemm_hybrid_reduce launch follows as before. */
  uint32_t* hybrid_counters; int32_t n_hybrid_counters;
  void* workspace;               /* fp32 scratch: [split_k, M, N] when split_k > 1; also enables the auto schedules */
  int64_t workspace_bytes;       /* (hybrid remainder split, skinny-N split-K) when tile == 0; may be NULL/0 */
} ovla_gemm_args;

/* The schedule `tile = 0` would pick for a dense GEMM (no skinny / small-M special case): tile id (17 = 256x256, 1 = 128x128,
 * 2 = 64x128, 5 = 128x32), how many tiles run whole, how many are split along K and how many ways, and the cost model's estimate.
 * (A launch that resolves to 17 runs the 256x256 tile's 4-wave configuration, id 18, when K >= 4096 is a multiple of 64, the LoRA rank is 0 or 32
 * and the epilogue is alpha / bias / residual only -- same tile grid, same remainder split, sums added in a different order.)
 * Host-only (no launch): lets callers and tests inspect the decision. */
int ovla_gemm_plan(int32_t M, int32_t N, int32_t K, int32_t K2, int32_t k2_group_n, int64_t workspace_bytes, int32_t* tile,
                   int32_t* full_tiles, int32_t* rem_tiles, int32_t* rem_splits, double* est_seconds);
/* The tile configuration ovla_gemm_bf16 would run for exactly these arguments (same checks, same decision code, no launch): what profilers and
 * bench.py use to name the kernel instance of a launch.  6 = the single-launch skinny kernel. */
int ovla_gemm_resolved_tile(const ovla_gemm_args* a, int32_t* tile);
int64_t ovla_gemm_workspace_bytes(int32_t M, int32_t N, int32_t split_k);
int ovla_gemm_bf16(const ovla_gemm_args* a, void* stream);

/* Batch-invariant GEMM: ovla_gemm_bf16's kernels under a schedule the CALLER fixes, so that the bits of an output row depend on
 * (N, K, K2, k2_group_n, epilogue) only -- never on M, on the row's tile or on how many rows share the launch.  Every output tile runs the
 * same way: whole (splits = 1), or split `splits` ways along K with the fp32 partial slabs summed in slab order and the epilogue applied by
 * the hybrid-remainder reduce (the same body as gemm_hybrid_reduce_kernel: no third arithmetic).  No hybrid full/remainder mix, no skinny or
 * small-M special case.  Batched inference (ops.batch_invariant) runs every forward GEMM through it.
 *   tile    1 (128x128), 2 (64x128), 5 (128x32), 17 (256x256), 18 (4-wave 256x256) or 22 (4-wave 128x256)
 *   splits  1 .. 8; splits * 4 K tiles of 64 must fit in K (the K-extension is not split) */
typedef struct {
  int32_t tile;
  int32_t splits;
} ovla_gemm_schedule;
/* Epilogue classes of ovla_gemm_fixed_schedule (bit flags): which tile configurations can run a problem. */
enum { OVLA_EPI_ROPE = 1,     /* rope_cos / rope_sin */
       OVLA_EPI_ROWSCALE = 2, /* rowscale_part (RMSNorm fold, consumer side) */
       OVLA_EPI_SWIGLU = 4,   /* act = OVLA_ACT_SWIGLU */
       OVLA_EPI_GENERAL = 8,  /* an activation, C_pre, colscale, FiLM, or a bias / residual operand not 16-byte aligned: 8-wave kernels only */
       OVLA_EPI_ROWSQ = 16    /* rowsq_out (RMSNorm fold, producer side) */ };
/* Host-only (no launch, no device query): the fixed schedule for a problem class, picked by the GEMM cost model over a ladder of row counts
 * (8 ... 9728: action-head rows up to a 16-observation decoder batch) as the one with the smallest summed slowdown against the best uniform
 * schedule at each row count.  The same (N, K, K2, k2_group_n, epi_flags) always gives the same schedule. */
int ovla_gemm_fixed_schedule(int32_t N, int32_t K, int32_t K2, int32_t k2_group_n, int32_t epi_flags, ovla_gemm_schedule* out);
/* fp32 workspace bytes ovla_gemm_bf16_fixed needs for M rows (0 when splits == 1): tiles * splits * tile_rows * tile_cols * 4. */
int64_t ovla_gemm_fixed_workspace_bytes(int32_t M, int32_t N, const ovla_gemm_schedule* s);
/* ovla_gemm_bf16 under schedule `s`.  `a->tile` and `a->split_k` must be 0 / <= 1, block-diagonal mode and the backward epilogues are not
 * supported; `a->workspace` must hold ovla_gemm_fixed_workspace_bytes.  A schedule whose tile cannot run the epilogue is OVLA_EINVAL. */
int ovla_gemm_bf16_fixed(const ovla_gemm_args* a, const ovla_gemm_schedule* s, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * "TN" GEMM (weight gradients)   C[P,Q] (+)= alpha * X[M,P]^T . Y[M,Q]     bf16 in, fp32 accumulate
 * Replaces autograd's weight-gradient matmuls for the trainable tensors: LoRA A/B (peft, finetune.py:862-871),
 * L1RegressionActionHead / ProprioProjector / NoisyActionProjector / FiLM Linears (finetune.py:894-932).
 * out_mode 0: fp32 accumulation into C (C must hold the running sum).  The M range is split over workgroups; with more than one split
 *             each writes its partial product to the fp32 workspace W ([splits, P, Q], ovla_gemm_tn_workspace_floats) and a second
 *             launch adds the partials to C in split order: the result is bit-reproducible run to run (no atomic order).
 *          1: fp32 store    2: bf16 store   (modes 1/2: no M split, W unused)
 */
typedef struct {
  const void* X; int64_t ldx;
  const void* Y; int64_t ldy;
  void* C; int64_t ldc;
  int32_t M, P, Q;
  float alpha;
  int32_t out_mode;
  float* W;
} ovla_gemm_tn_args;
/* fp32 elements of W the problem needs when launched alone (group_size 1) or as one of group_size problems of ovla_gemm_tn_grouped. */
int64_t ovla_gemm_tn_workspace_floats(const ovla_gemm_tn_args* a, int32_t group_size);
int ovla_gemm_tn_bf16(const ovla_gemm_tn_args* a, void* stream);
/* Up to OVLA_TN_MAX_GROUP independent TN problems in ONE launch (the dA / dB_g products of one LoRA linear): the small
 * problems then overlap on the chip instead of running back to back. */
#define OVLA_TN_MAX_GROUP 4
int ovla_gemm_tn_grouped(const ovla_gemm_tn_args* problems, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Multi-adapter serving: n LoRA adapters ("slots", one per fine-tuned policy) in ONE K-extended GEMM launch.  peft applies one adapter per
 * model, `result + lora_B(lora_A(x)) * scaling` (finetune.py:862-871); here the projection GEMM runs against the n adapters' stacked A
 * (t [M, G*n*r], group-major: group g owns columns [g n r, (g+1) n r), slot s inside it [s r, (s+1) r)) and ovla_lora_route then stores bf16 +0
 * over every column block of a slot other than the row's own, so the K-extension (K2 = n r, k2_group_n as before) adds exactly the row's own
 * adapter: zeros contribute nothing to the fp32 accumulator.  Row m belongs to observation m / rows_per_obs, whose slot is obs_slot[obs]
 * (DEVICE int32 [n_obs]: a captured graph serves any assignment).  Zeros are STORED, never multiplied in: a non-finite value in a foreign
 * adapter's projection does not reach the row.  The row's own columns and the columns >= G*n*r (ld padding) are left untouched.  16-byte
 * vector stores, no atomics, stream-ordered and capturable; r % 8 == 0, ld % 8 == 0, ld >= G*n*r, 16-byte aligned t, n_obs * rows_per_obs >= M.
 * obs_slot_host (optional): the same n_obs values in HOST memory; an entry outside [0, n) is OVLA_EINVAL before anything is launched.  The
 * kernel itself clamps what it reads from the device array to [0, n): it never reads or writes out of range.  n == 1 launches nothing. */
typedef struct {
  void* t; int64_t ld;               /* bf16 [M, ld], routed in place */
  const int32_t* obs_slot;           /* device int32 [n_obs] */
  const int32_t* obs_slot_host;      /* optional host copy, validated */
  int32_t M, G, n, r, rows_per_obs, n_obs;
} ovla_lora_route_args;
int ovla_lora_route(const ovla_lora_route_args* a, void* stream);

/* dst[m, :] = src[slot(m), m, :]: each observation's own policy's output out of n stacked candidates -- the per-policy L1 action heads'
 * predictions (prismatic/models/action_heads.py:84-107; a fine-tune saves its own `action_head--*.pt`, finetune.py:584-675) and proprio
 * projectors' tokens (prismatic/models/projectors.py:6-24), computed for all observations by every registered policy and picked here.
 * src [n, rows, dim] with src_slot_stride elements between slots (0: rows * dim), dst [rows, dim] contiguous, elem_bytes 2 (bf16) or 4 (fp32);
 * slot(m) = obs_slot[m / rows_per_obs] with ovla_lora_route's addressing, host validation (obs_slot_host) and device-side clamp. */
typedef struct {
  const void* src; void* dst;
  const int32_t* obs_slot; const int32_t* obs_slot_host;
  int64_t src_slot_stride;
  int32_t n, rows, dim, rows_per_obs, n_obs, elem_bytes;
} ovla_select_by_slot_args;
int ovla_select_by_slot(const ovla_select_by_slot_args* a, void* stream);

/* Per-policy FiLM: every observation's gamma / beta vectors from ITS OWN policy's scale / shift Linears (prismatic/models/film_vit_wrapper.py:53-54,
 * 65-72: `gamma = self.scale(average_language_embedding)`, `beta = self.shift(...)` in every tower block; a fine-tune saves them inside
 * `vision_backbone--{step}_checkpoint.pt`, experiments/robot/openvla_utils.py:311-349), for all n_linears Linears of both towers in ONE launch:
 *     out_j[b, c] = bf16( bias_j[slot(b)][c] + sum_k W_j[slot(b)][c, k] * avg[b, k] )        b < n_obs, fp32 sums, one rounding
 * with slot(b) = obs_slot[b] (DEVICE int32 [n_obs], clamped to [0, n) by the kernel as ovla_lora_route clamps: no index formed from it leaves a
 * buffer; obs_slot_host, optional, is validated before anything is launched).  Linear j is one ovla_film_linear:
 *     W bf16 [n][out_f][D] (16-byte base), bias bf16 [n][out_f], out bf16 [rows >= n_obs][out_f] (row stride out_f), out_f >= 1,
 *     item_start = sum over the Linears before j of ceil(out_f / OVLA_FILM_ITEM_COLS)   (a wave computes OVLA_FILM_ITEM_COLS columns at a time)
 * `table` is the DEVICE array of the n_linears descriptors, `table_host` the same array in HOST memory (validated: pointers, out_f, alignment,
 * item_start).  avg bf16 [>= n_obs, D] with row stride ld_avg (elements; % 8, 16-byte base).  D % 8 == 0 (any such D whose row fits in LDS),
 * 1 <= n <= OVLA_MAX_SLOTS, 1 <= n_obs <= OVLA_FILM_MAX_OBS.
 *  - Only the slots some observation is routed to are read: an unused slot's weights may be stale or NaN.  Rows >= n_obs of every out are not
 *    written.  A row's arithmetic sees its own avg row and its own slot's weights only (selected by address, never multiplied by 0 / 1).
 *  - Batch-invariant by construction: a lane adds its 16-byte k-vectors l, l + 64, ... in order, the 64 lane sums meet in one fixed exchange tree;
 *    the bits of out_j[b, :] depend on avg[b, :], the weights of slot(b), D and out_f -- not on n_obs, b's position, the other observations or n.
 *  - Each weight row is streamed once per used slot and group of 8 observations of that slot (16-byte loads straight to registers, 4 rows per
 *    wave in flight, the group's avg rows staged in LDS); no atomics, no cross-workgroup communication; stream-ordered and capturable.
 * Every argument check returns OVLA_EINVAL before any launch. */
#define OVLA_MAX_SLOTS 4
#define OVLA_FILM_MAX_OBS 64
#define OVLA_FILM_ITEM_COLS 4
typedef struct { const void* W; const void* bias; void* out; int32_t out_f; int32_t item_start; } ovla_film_linear;
typedef struct {
  const void* table;                 /* device ovla_film_linear [n_linears] */
  const void* table_host;            /* the same descriptors in host memory */
  const void* avg; int64_t ld_avg;   /* bf16 [>= n_obs, D] */
  const int32_t* obs_slot;           /* device int32 [n_obs] */
  const int32_t* obs_slot_host;      /* optional host copy, validated */
  int32_t n_linears, n_obs, n, D;
} ovla_film_vectors_args;
int ovla_film_vectors(const ovla_film_vectors_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * LoRA dropout (FinetuneConfig.lora_dropout, finetune.py:119 -> LoraConfig, :862-871): peft puts an independent nn.Dropout(p) in front of the
 * lora_A of every adapted nn.Linear, active in training mode only:  y = W x + s B_g(A_g(dropout_g(x))).  A fused q|k|v or gate|up linear
 * therefore has one mask per fused group.  Here the mask is a pure function of (seed, call, module, row, column), evaluated in registers by
 * whichever kernel holds the element; it is never stored.  THE MASK CONTRACT (identical in the three kernels below and in the numpy
 * restatement tests/lora_dropout_reference.py):
 *   generator   Philox4x32-10, multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85.
 *   call        one generator call per 16-byte vector = 8 consecutive columns of one row: q = m * (K / 8) + (k >> 3) as a 64-bit number,
 *               counter (q_lo, q_hi, module, call), key (seed_lo, seed_hi).  Output word w gives column 8 (k >> 3) + 2 w from its low 16 bits
 *               and column 8 (k >> 3) + 2 w + 1 from its high 16 bits.
 *   keep rule   keep iff u16 >= thr, thr = floor(p * 65536) with p the fp32 argument widened to double: the drop probability is exactly
 *               thr / 65536.  0 <= p < 1, K % 8 == 0.
 *   indexing    m, k are the logical row and column of the linear's own input matrix [M, K]; the mask does not depend on a leading dimension,
 *               on launch geometry or on which kernel evaluates it.  `module` is a caller-chosen 32-bit id per adapted sub-linear, `call` a
 *               32-bit counter the caller advances once per training forward.
 *   scale       inv = 1.0f / (1.0f - p) in fp32 (IEEE division, no contraction).  A kept element is bf16_rne(float(x) * inv); a dropped
 *               element is STORED as +0, never multiplied, so a NaN in a dropped position does not survive (ovla_lora_route's convention).
 * All three entry points are stream-ordered and capturable, use no atomics (t and dx feed the bit-reproducible gradient chain) and launch
 * nothing on OVLA_EINVAL.  G <= 4 groups; module[g] for g < G. */

/* out[g][m, k] = dropout_g(x)[m, k]: G contiguous [M, K] bf16 buffers from ONE read of x [M, K] (row stride ldx).  Columns >= K of x are not
 * read.  K % 8 == 0, ldx % 8 == 0, 16-byte aligned x and out[g], out[g] != x. */
typedef struct {
  const void* x; int64_t ldx;
  void* out[4];
  uint32_t module[4];
  uint32_t seed_lo, seed_hi, call;
  float p;
  int32_t M, K, G;
} ovla_lora_dropout_apply_args;
int ovla_lora_dropout_apply(const ovla_lora_dropout_apply_args* a, void* stream);

/* t[m, g r + j] = bf16(alpha * sum_k dropout_g(x)[m, k] * A[g r + j, k]) for all G groups in one launch; r == 32, fp32 accumulation, the K
 * split over a workgroup's 4 waves is reduced through LDS in wave order (run-to-run bit-identical).  x [M, K] (ldx), A [G r, K] (lda),
 * t [M, G r] (ldt; columns >= G r untouched).  K % 8 == 0, ldx % 8 == 0, lda % 8 == 0, ldt % 4 == 0, x and A 16-byte, t 8-byte aligned. */
typedef struct {
  const void* x; int64_t ldx;
  const void* A; int64_t lda;
  void* t; int64_t ldt;
  uint32_t module[4];
  uint32_t seed_lo, seed_hi, call;
  float p, alpha;
  int32_t M, K, G, r;
} ovla_lora_dropout_proj_args;
int ovla_lora_dropout_proj(const ovla_lora_dropout_proj_args* a, void* stream);

/* In place on dx [M, K] (ld; columns >= K untouched):
 *   dx[m, k] = bf16(float(dx[m, k]) + sum_g (keep_g(m, k) ? inv * acc_g[m, k] : 0)),  acc_g[m, k] = sum_j dt[m, g r + j] * AT[k, g r + j] in fp32,
 * the sum over g in group order, one rounding.  dt [M, G r] (ld_dt), AT [K, G r] (ld_at) = A^T.  r % 8 == 0, r <= 128 (fragments are
 * zero-padded to the MFMA's K in registers), K % 8 == 0, every ld % 8 == 0, 16-byte aligned bases. */
typedef struct {
  void* dx; int64_t ld;
  const void* dt; int64_t ld_dt;
  const void* AT; int64_t ld_at;
  uint32_t module[4];
  uint32_t seed_lo, seed_hi, call;
  float p;
  int32_t M, K, G, r;
} ovla_lora_dropout_backproj_args;
int ovla_lora_dropout_backproj(const ovla_lora_dropout_backproj_args* a, void* stream);

/* column sums  out[n] (+)= sum_m X[m,n]   (bias gradients).  out fp32, atomic accumulate. */
typedef struct { const void* X; int64_t ldx; float* out; int32_t M, N; } ovla_colsum_args;
int ovla_colsum_bf16(const ovla_colsum_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Attention (no KV paging; whole short context; K/V tiles staged through LDS)
 *   O[b,s,h,:] = softmax_k( scale * Q[b,s,h,:] . K[b,k,h,:]  + mask ) V[b,k,h,:]
 * Replaces F.scaled_dot_product_attention inside timm Attention (ViT, unmasked) and inside the transformers-fork
 * LlamaAttention (bidirectional + key padding: reference pyproject.toml:50, modeling_prismatic.py:742; `causal`
 * selects the stock lower-triangular mask).  Key padding is right padding only (reference collator
 * prismatic/util/data_utils.py:115): keys >= kv_len[b] are masked; kv_len == NULL means all S keys.
 * Q/K/V/O are addressed as  base + (b*S + s) * row_stride + h * head_dim  (elements), so the fused QKV GEMM output is
 * consumed in place.  head_dim in {64, 72, 128}.  lse: fp32 [B, H, S] (natural-log sum-exp of the scaled scores).
 */
typedef struct {
  const void* Q; const void* K; const void* V; int64_t q_stride, k_stride, v_stride;
  void* O; int64_t o_stride;
  float* lse;
  const int32_t* kv_len;  /* optional [B] */
  int32_t B, H, S, head_dim;
  int32_t causal;
  float scale;
} ovla_attn_fwd_args;
int ovla_attn_fwd(const ovla_attn_fwd_args* a, void* stream);

typedef struct {
  const void* Q; const void* K; const void* V; int64_t q_stride, k_stride, v_stride;
  const void* O; const void* dO; int64_t o_stride, do_stride;
  const float* lse;
  float* delta;            /* workspace fp32 [B,H,S]: rowsum(dO * O), written by the dQ kernel, read by the dK / dV kernel */
  void* dQ; void* dK; void* dV; int64_t dq_stride, dk_stride, dv_stride;
  const int32_t* kv_len;
  int32_t B, H, S, head_dim;
  int32_t causal;
  float scale;
  const void* rope_cos;    /* optional bf16 [S, head_dim/2] tables (ovla_rope_table): dQ and dK are written with the INVERSE RoPE rotation */
  const void* rope_sin;    /* applied (the gradient w.r.t. the pre-RoPE q / k: saves the separate ovla_rope(inverse) pass); head_dim 128 */
} ovla_attn_bwd_args;
int ovla_attn_bwd(const ovla_attn_bwd_args* a, void* stream);

/* Attention probabilities of a list of query rows (output_attentions): read-only, recomputed from what ovla_attn_fwd consumed and wrote.
 *   visible key:  P[r,h,k] = exp2( fp32(Q[row r,h,:] . K[b,k,h,:]) * (scale * log2e) - lse[b,h,s] * log2e )   (the backward kernels' expression)
 *   masked key (k >= kv_len[b], or with `causal` k > s):  exactly 0.0f, by select -- a NaN in a masked K row does not reach the output
 *   P_mean[r,k] = acc * (1.0f / H),  acc summed over h = 0 .. H-1 in that order in fp32 (no atomics: the same bits on every run)
 * rows[r] = b*S + s is device memory and is range-checked before use: an index outside [0, B*S) writes a zero row and reads nothing.  A
 * row's result depends on its own q row, its batch entry's K, lse and kv_len only -- not on R, on its position in the list or on B.
 * head_dim in {64, 128} (the towers' 72 is refused); Q / K 16-byte aligned with row strides that are multiples of 8 elements; R > 0; at
 * least one of P and P_mean.  Anything else returns OVLA_EINVAL with a message and launches nothing.
 */
typedef struct {
  const void* Q; const void* K; int64_t q_stride, k_stride;  /* addressed exactly as in ovla_attn_fwd_args (post-RoPE, heads contiguous) */
  const float* lse;        /* fp32 [B,H,S]: what ovla_attn_fwd wrote for the same Q, K, kv_len, causal, scale */
  const int32_t* kv_len;   /* optional [B] */
  const int32_t* rows;     /* int32 [R] flattened query rows b*S+s (the convention of LlamaStack.fwd's `sel` and of action_rows): any order,
                              repeats allowed; NULL: R == B*S and row r is r */
  float* P;                /* optional fp32 [R, H, S] */
  float* P_mean;           /* optional fp32 [R, S]: mean over heads */
  int32_t B, H, S, R, head_dim, causal; float scale;
} ovla_attn_probs_args;
int ovla_attn_probs(const ovla_attn_probs_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Normalisation.  RMSNorm: transformers LlamaRMSNorm (fp32 math, eps 1e-5).  LayerNorm: timm blocks (eps 1e-6) and
 * MLPResNet (action_heads.py:64,69, eps 1e-5).  x/y bf16 [rows, dim]; weight/bias bf16 [dim] (bias NULL for RMS).
 * rstd (and mean) fp32 [rows] are saved for the backward.  The backward returns dx (bf16); dw/db (fp32, atomic
 * accumulate) only when non-NULL (they are frozen on the LoRA path except in the action head).
 * If `dx_accum` != 0 the backward ADDS into dx (residual-stream gradient) instead of overwriting it.
 */
typedef struct {
  const void* x; void* y; const void* weight; const void* bias;
  float* mean; float* rstd;
  int32_t rows, dim; float eps; int32_t is_rms;
} ovla_norm_fwd_args;
int ovla_norm_fwd(const ovla_norm_fwd_args* a, void* stream);

typedef struct {
  const void* x; const void* dy; const void* weight;
  const float* mean; const float* rstd;
  void* dx; float* dweight; float* dbias;
  int32_t rows, dim; int32_t is_rms; int32_t dx_accum;
} ovla_norm_bwd_args;
int ovla_norm_bwd(const ovla_norm_bwd_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * RoPE, in place on the q and k heads of a fused [rows, ld] buffer (HF "rotate_half" convention; position = row % S).
 * cos/sin tables are bf16 [S, head_dim/2], built once by ovla_rope_table (fp32 angles, then cast to bf16 exactly as
 * transformers LlamaRotaryEmbedding does before apply_rotary_pos_emb).  `inverse` applies the transposed rotation
 * (backward).  n_heads = q heads + k heads, contiguous from column 0.
 */
int ovla_rope_table(void* cos_table, void* sin_table, int32_t S, int32_t head_dim, float theta, void* stream);
typedef struct {
  void* qk; int64_t ld; int32_t rows, S, n_heads, head_dim;
  const void* cos_table; const void* sin_table; int32_t inverse;
} ovla_rope_args;
int ovla_rope(const ovla_rope_args* a, void* stream);

/* SwiGLU:  h = silu(g) * u  with gu = [g | u] as [rows, 2F];  backward writes dgu from dh and gu. */
typedef struct { const void* gu; void* h; int32_t rows, F; } ovla_swiglu_fwd_args;
int ovla_swiglu_fwd(const ovla_swiglu_fwd_args* a, void* stream);
typedef struct { const void* gu; const void* dh; void* dgu; int32_t rows, F; } ovla_swiglu_bwd_args;
int ovla_swiglu_bwd(const ovla_swiglu_bwd_args* a, void* stream);

/* activation backward:  dz = dh * act'(z)   (z = saved pre-activation), elementwise on [n] bf16 */
typedef struct { const void* z; const void* dh; void* dz; int64_t n; int32_t act; } ovla_act_bwd_args;
int ovla_act_bwd(const ovla_act_bwd_args* a, void* stream);

/* y = alpha*x (+ y if accum)   and friends: small elementwise helpers on bf16 buffers */
typedef struct { const void* a; const void* b; void* out; int64_t n; } ovla_add_args;
int ovla_add_bf16(const ovla_add_args* a, void* stream);  /* out = a + b (b may be NULL: copy) */
typedef struct { const void* x; const void* scale; void* out; int32_t rows, dim; } ovla_colscale_args;
int ovla_colscale_bf16(const ovla_colscale_args* a, void* stream); /* out[m,n] = x[m,n]*scale[n] */

/* ------------------------------------------------------------------------------------------------------------------
 * Vision front end.
 * im2col for the 14x14/stride-14 patch embedding (timm PatchEmbed Conv2d as GEMM): pixel_values bf16 NCHW
 * [B, C_total, H, W]; image `img` (0..n_img-1) of a batch row uses channels [c0 + img*img_cstride, +3)
 * (modeling_prismatic.py:210-224: 6 channels per image, DINOv2 first, SigLIP second) -> rows [(B*n_img)*gh*gw, ldo] with
 * K = 3*p*p real columns (c, py, px) and zero pad.  n_img == 0 means 1.
 */
typedef struct { const void* pixels; void* out; int64_t ldo; int32_t B, C_total, c0, H, W, patch, n_img, img_cstride; } ovla_im2col_args;
int ovla_im2col(const ovla_im2col_args* a, void* stream);

/* Inference-side image preparation as ONE kernel (experiments/robot/openvla_utils.py:542-622 `center_crop_image`:
 * convert_image_dtype(u8 -> f32) = x * (1/255); tf.image.crop_and_resize of the central sqrt(crop_scale) box back to out x out
 * (TF 2.15 CropAndResize arithmetic in fp32: in_y = y1 (H-1) + i (y2-y1)(H-1)/(out-1), lerp form a + (b-a) w); clip; back to uint8
 * as trunc(x * 255.5); then prismatic/extern/hf/processing_prismatic.py:128-145 `apply_transform`: to_tensor (/255) and
 * per-backbone normalise, channel-stacked).  src uint8 [n_img, H, W, 3] (HWC, device) -> dst bf16 [n_img * 6, out, out]:
 * image i -> channels [6 i, 6 i + 3) normalised with mean[0..2]/std[0..2] (DINOv2) and [6 i + 3, 6 i + 6) with mean[3..5]/std[3..5]
 * (SigLIP).  crop == 0: the pixels are taken as they are (requires H == W == out).  Every fp32 operation is individually
 * rounded (no FMA contraction): bit-exact against the host restatement (image_prep.center_crop_image + apply_transform). */
typedef struct { const void* src; void* dst; int32_t n_img, H, W, out, crop; float crop_scale; float mean[6]; float std[6]; } ovla_image_prep_args;
int ovla_image_prep(const ovla_image_prep_args* a, void* stream);

/* Separable resampling with per-output-pixel spans (TF 2.15 `scale_and_translate_op.cc`, the kernel behind
 * tf.image.resize(method="lanczos3", antialias=True) that experiments/robot/openvla_utils.py:516-540 `resize_image_for_policy` and
 * dlimp's `resize_image` (rlds/obs_transforms.py:83) call): rows first into an fp32 intermediate [n, out_h, W, 3], then columns;
 * out = sum_k weights[o, k] * in[starts[o] + k] accumulated in span order from 0, each multiply and add rounded on its own; then
 * tf.round (half to even), clip to [0, 255], uint8.  The spans (starts int32 [out], weights fp32 [out, span]) are computed by the host
 * (image_prep.lanczos3_spans) and passed as device arrays.  The reference's JPEG encode/decode round trip before the resize is
 * ovla_jpeg_roundtrip below; PARITY UNPINNED against TensorFlow, bit-compared with oracle/data_oracle.py. */
typedef struct {
  const void* src; void* dst; void* workspace; int64_t workspace_bytes;
  const int32_t* row_starts; const float* row_weights; const int32_t* col_starts; const float* col_weights;
  int32_t n_img, H, W, out_h, out_w, row_span, col_span;
} ovla_image_resize_args;
int64_t ovla_image_resize_workspace_bytes(int32_t n_img, int32_t W, int32_t out_h);
int ovla_image_resize(const ovla_image_resize_args* a, void* stream);

/* The JPEG encode -> decode round trip of `resize_image_for_policy` (experiments/robot/openvla_utils.py:532-533: tf.image.encode_jpeg(img)
 * then tf.io.decode_image(...), default arguments = libjpeg-turbo baseline 4:2:0 at quality 95, accurate integer DCT, fancy upsampling) as
 * two launches, without the (lossless) entropy coder: per 16 x 16 MCU RGB -> YCbCr, 2x2 chroma box filter, 8x8 forward DCT, quantise,
 * dequantise, inverse DCT -> component planes in `workspace`; then triangle-filter chroma upsampling + YCbCr -> RGB per pixel.  Integer
 * arithmetic throughout, bit-identical to oracle/jpeg_oracle.py, which is pinned to libjpeg-turbo's own output (tests/golden/g12).
 * src / dst uint8 [n_img, H, W, 3] (any H, W >= 1: edges are padded by replication as the library does); quality 1..100. */
typedef struct { const void* src; void* dst; void* workspace; int64_t workspace_bytes; int32_t n_img, H, W, quality; } ovla_jpeg_roundtrip_args;
int64_t ovla_jpeg_roundtrip_workspace_bytes(int32_t n_img, int32_t H, int32_t W);
int ovla_jpeg_roundtrip(const ovla_jpeg_roundtrip_args* a, void* stream);

/* Training-time image path as two launches (replaces the TF/dlimp frame transform + PIL/torchvision processor of the reference's data
 * loader: prismatic/vla/datasets/rlds/obs_transforms.py:18-45 `augment` -> dlimp `augment_image` with the kwargs of
 * prismatic/vla/datasets/datasets.py:159-174, then prismatic/extern/hf/processing_prismatic.py:128-145 `apply_transform`).
 * Per image, fp32, every operation individually rounded (no FMA contraction), `clip(0, 1)` after every enabled op:
 *   x = u8 / 255
 *   bit 0  crop_and_resize(box = params[0..3] = y1, x1, y2, x2, to out x out)   TF CropAndResize, bilinear, extrapolation 0
 *   bit 1  x + params[4]                                                        tf.image.adjust_brightness
 *   bit 2  (x - mean_c) * params[5] + mean_c, mean over the image per channel   AdjustContrastv2 (mean accumulated in fp64 here)
 *   bit 3  rgb -> hsv, s = clamp(s * params[6], 0, 1), hsv -> rgb                adjust_saturation_op.cc (CPU kernel arithmetic)
 *   bit 4  rgb -> (h, v_min, v_max), h += 6 * params[7] wrapped to [0, 6), back  adjust_hue_op.cc (CPU kernel arithmetic)
 *   u8 = trunc(x * 255); then to_tensor (/255) and the two backbones' normalisations as in ovla_image_prep.
 * ops_mask == 0 is the evaluation path (quantise + normalise only; H == W == out required unless bit 0 is set).
 * src uint8 [n_img, H, W, 3] (device) ; params fp32 [n_img, 8] (device) ; dst bf16 [n_img, 6, out, out] ;
 * workspace: ovla_image_augment_workspace_bytes(n_img, out) bytes (fp32 intermediate image + per-block fp64 channel sums).
 * TensorFlow / dlimp are not available offline: PARITY UNPINNED against TF, bit-compared with oracle/data_oracle.py. */
typedef struct {
  const void* src; void* dst; const float* params; void* workspace; int64_t workspace_bytes;
  int32_t n_img, H, W, out, ops_mask; float mean[6]; float std[6];
} ovla_image_augment_args;
int64_t ovla_image_augment_workspace_bytes(int32_t n_img, int32_t out);
int ovla_image_augment(const ovla_image_augment_args* a, void* stream);

/* tokens[b, pre + i, :] = patches[b, i, :] + pos[i, :] ;  tokens[b, j, :] = prefix[j, :]  (cls / register tokens)
 * (timm VisionTransformer._pos_embed with no_embed_class=True) */
typedef struct { const void* patches; const void* pos; const void* prefix; void* tokens; int32_t B, n_patches, n_prefix, dim; } ovla_vit_embed_args;
int ovla_vit_embed(const ovla_vit_embed_args* a, void* stream);
/* strided row copy: dst[b, i, dst_col0 : dst_col0+dim] = src[b, src_row0 + i, :]   (drop prefix tokens + feature concat,
 * modeling_prismatic.py:221-227); `accumulate` adds instead (used by the backward). */
typedef struct {
  const void* src; void* dst; int32_t B, rows, dim;
  int64_t src_batch_stride, src_row0, src_ld, dst_batch_stride, dst_row0, dst_ld, dst_col0; int32_t accumulate;
} ovla_copy_rows_args;
int ovla_copy_rows(const ovla_copy_rows_args* a, void* stream);

/* FiLM backward (prismatic/models/film_vit_wrapper.py:72: x = x_pre * (1 + gamma[b]) + beta[b], b = row / rows_per_batch):
 *   dgamma[b,n] += sum_rows dy * x_pre ;  dbeta[b,n] += sum_rows dy ;  dy <- dy * (1 + gamma[b,n])   (in place)
 * dgamma / dbeta fp32 [B, dim] (accumulated), gamma bf16 [B, dim]. */
typedef struct { void* dy; const void* x_pre; const void* gamma; float* dgamma; float* dbeta; int32_t B, rows_per_batch, dim; } ovla_film_bwd_args;
int ovla_film_bwd(const ovla_film_bwd_args* a, void* stream);

/* mean pooling:  out[b,:] = mean over rows i with row_mask[b,i] != 0 of x[b, i, :]  (FiLM's average language embedding) */
typedef struct { const void* x; const uint8_t* row_mask; void* out; int32_t B, L, dim; } ovla_masked_mean_args;
int ovla_masked_mean(const ovla_masked_mean_args* a, void* stream);

/* FiLM's conditioning vector straight from the token ids (modeling_prismatic.py:575-583: `input_embeddings[~all_actions_mask]`
 * averaged over the sequence, film_vit_wrapper.py:243): out[b,:] = bf16(mean_i embed[ids[b,i], :]) over the text positions i whose label
 * is NOT an action token (labels[b,i] <= action_token_begin, which includes IGNORE_INDEX: BOS, prompt, stop and pad positions all
 * count, as in the reference).  The action mask is the same integer rule as ovla_assemble_multimodal's (an action token is always a
 * counted label, so the cumulative-count clause of train_utils.py:8-39 cannot change it).  fp32 sum of the bf16 rows, one rounding.
 * ids / labels int64 [B, L]; embed bf16 [vocab, D]; out bf16 [B, D].  No host synchronisation: capturable in a hipGraph. */
typedef struct { const int64_t* ids; const int64_t* labels; const void* embed_table; void* out; int32_t B, L, D, vocab; int64_t action_token_begin; } ovla_language_average_args;
int ovla_language_average(const ovla_language_average_args* a, void* stream);

/* The same vector for a right-padded batch in ONE launch: row b averages the positions i < lens[b] only (lens int32 [B] on the device, each
 * in [1, L]), otherwise the rule above.  out[b,:] is bit for bit what ovla_language_average returns for the single row ids[b, :lens[b]],
 * labels[b, :lens[b]] (same fp32 summation order, one rounding), so pad tokens never enter a prompt's mean and the batched FiLM forward is
 * capturable too (engine.ChunkGraph(film=True)). */
typedef struct { const int64_t* ids; const int64_t* labels; const int32_t* lens; const void* embed_table; void* out; int32_t B, L, D, vocab; int64_t action_token_begin; } ovla_language_average_ragged_args;
int ovla_language_average_ragged(const ovla_language_average_ragged_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Multimodal sequence assembly (modeling_prismatic.py:571-629): one pass writes
 *   out[b, 0]            = embed[ids[b,0]]
 *   out[b, 1 .. P]       = patches[b, :]            (P = projected patches + proprio (+ timestep) tokens)
 *   out[b, P+1+i]        = action_mask[b,1+i] ? (noisy ? noisy[b, slot] : 0) : embed[ids[b, 1+i]]
 * action_mask is computed on device from labels exactly as train_utils.get_current_action_mask | get_next_actions_mask
 * (cumsum of labels != -100, labels > 31743); `action_pos` receives, per batch row and action slot, the flattened row
 * b*(P+L) + (P + i) - 1 of the assembled sequence whose final hidden state PREDICTS that slot (i = text index of the
 * slot; shift-by-one of finetune.py:385-394 / modeling_prismatic.py:915-920), ready for ovla_gather_rows.
 */
typedef struct {
  const int64_t* ids; const int64_t* labels;   /* [B, L] */
  const void* embed_table;                      /* bf16 [V, D] */
  const void* patches;                          /* bf16 [B, P, D] */
  const void* noisy;                            /* optional bf16 [B, A, D] */
  void* out;                                    /* bf16 [B, P+L, D] */
  int32_t* action_pos;                          /* optional int32 [B, A]: predicting row of each action slot */
  int32_t B, L, P, D, A, vocab;
  int32_t ignore_index, action_token_begin, action_dim;
} ovla_assemble_args;
int ovla_assemble_multimodal(const ovla_assemble_args* a, void* stream);

/* Per-row sums of squares of every 64-column group: out[m, j] = sum x[m, 64 j .. 64 j + 63]^2 (fp32, [rows, dim / 64]) -- the RMSNorm-fold
 * input of the FIRST decoder layer (ovla_gemm_args.rowscale_part); later layers get theirs from the producing GEMM's epilogue (rowsq_out). */
int ovla_row_sumsq(const void* x, int64_t ld, float* out, int32_t rows, int32_t dim, void* stream);

/* dst[i, :] = src[index[i], :]  /  scatter-add backward dst[index[i], :] += src[i, :].
 * An index < 0 means "no row" (ovla_assemble_multimodal leaves -1 in action_pos for an action slot the labels do not hold, and the labels
 * may be device-resident, where no host check sees them): the gather writes a ZERO row at i, the scatter-add skips entry i.  Nothing is
 * read or written outside src / dst for it.  An index beyond the last row is the caller's to exclude: the row count is not an argument. */
typedef struct { const void* src; const int32_t* index; void* dst; int32_t n, dim; int64_t src_ld, dst_ld; int32_t scatter_add; } ovla_gather_rows_args;
int ovla_gather_rows(const ovla_gather_rows_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * L1 action head tail (prismatic/models/action_heads.py:69-81, finetune.py:400):
 *   pred[m, :adim] = x[m,:] . W[adim, dim]^T + b ;  loss = mean |pred - target|
 * and its backward (dpred = sign(pred-target)/count * dloss -> dx, dW, db).  The wide layers of the head run on
 * ovla_gemm_bf16 / ovla_norm_*; this is the N = ACTION_DIM tail that does not fit an MFMA tile.
 */
/* Next-token cross entropy on selected rows (the discrete action-token objective: vla-scripts/finetune.py:357-359 `loss =
 * output.loss`, i.e. the transformers LlamaForCausalLM loss: logits.float(), shift by one, CrossEntropyLoss(ignore_index=-100,
 * mean) -- the caller gathers the rows whose shifted label is not ignored, so only those rows reach lm_head).
 * logits bf16 [rows, ld] (read as fp32, as `.float()` does) ; targets int64 [rows] in [0, vocab)
 *   loss_rows[r] = logsumexp(logits[r, :vocab]) - logits[r, target[r]]   (fp32)
 *   argmax[r]    = lowest index of the row maximum                       (predicted_token_ids, finetune.py:358); 0 for a row that is all -inf or only NaN
 *   dlogits[r,j] = bf16((softmax(logits[r])[j] - [j == target[r]]) * grad_scale)   (optional; may alias logits)
 * grad_scale = loss_scale / number of non-ignored tokens in the batch (the mean's 1/N and the grad-accumulation divide). */
typedef struct {
  const void* logits; int64_t ld; const int64_t* targets; float* loss_rows; int32_t* argmax; void* dlogits; int64_t ld_d;
  int32_t rows, vocab; float grad_scale;
} ovla_token_ce_args;
int ovla_token_ce(const ovla_token_ce_args* a, void* stream);

/* Greedy decode of the discrete action tokens (modeling_prismatic.py:929-942: `logits.argmax(dim=2)`, then
 * `np.clip(vocab_size - ids - 1, 0, bin_centers.shape[0] - 1)`), on the device so that it can sit inside a captured graph:
 *   token[r] = lowest index of the maximum of logits[r, 0 .. vocab)          (the tie rule of ovla_token_ce's argmax)
 *   bin[r]   = clip(n_tokens - token[r] - 1, 0, n_bins - 1)
 * logits bf16 [rows, ld], ld >= vocab, values finite or -inf; columns [vocab, ld) are never read.  token / bin int32 [rows].  The float64
 * bin-centre lookup and the un-normalisation stay on the host. */
typedef struct { const void* logits; int64_t ld; int32_t* token; int32_t* bin; int32_t rows, vocab, n_tokens, n_bins; } ovla_argmax_bins_args;
int ovla_argmax_bins(const ovla_argmax_bins_args* a, void* stream);

typedef struct {
  const void* x; const void* W; const void* b; void* pred;   /* bf16 */
  const void* target; float* loss_sum;                        /* optional: accumulates sum |pred-target| (or squared, mse) */
  int32_t rows, dim, adim;
  int32_t mse;
} ovla_head_out_fwd_args;
int ovla_head_out_fwd(const ovla_head_out_fwd_args* a, void* stream);
typedef struct {
  const void* x; const void* W; const void* pred; const void* target;
  const void* dpred;            /* optional bf16 [rows, adim]: explicit upstream gradient (pred/target/mse then ignored) */
  float dloss_scale;            /* dloss / (rows*adim) */
  int32_t mse;                  /* 0: L1 (sign), 1: MSE (2*(pred-target)) */
  void* dx; float* dW; float* db;
  int32_t rows, dim, adim;
} ovla_head_out_bwd_args;
int ovla_head_out_bwd(const ovla_head_out_bwd_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Fused AdamW over a flat parameter buffer (torch.optim.AdamW as called at finetune.py:952: betas (0.9,0.999),
 * eps 1e-8, weight_decay 0.01).  bf16 variant reproduces torch's per-op bf16 rounding sequence
 * (param *= 1-lr*wd; m.lerp_(g,1-b1); v = v*b2 + (1-b2) g*g; denom = sqrt(v)/sqrt(bc2) + eps; p -= (lr/bc1) m/denom)
 * so results are bit-identical to torch on the same inputs.  grads are fp32 master-accumulated here and are rounded to
 * the parameter dtype first (what autograd would have stored).  grad_scale multiplies the gradient (1/world, 1/accum).
 */
typedef struct {
  void* param; void* exp_avg; void* exp_avg_sq;   /* bf16 or fp32 (is_bf16) */
  const float* grad;
  int64_t n; int32_t is_bf16; int32_t step;       /* step >= 1 (after increment, as torch) */
  double lr, beta1, beta2, eps, weight_decay;     /* Python floats, combined in double like torch/optim/adamw.py */
  float grad_scale;
} ovla_adamw_args;
int ovla_adamw(const ovla_adamw_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Weight EMA: the exponential moving average of a flat parameter buffer, kept in an fp32 shadow and updated right after the optimizer
 * step (vla-scripts/finetune.py:952 is where the reference builds its optimizer; the reference has NO EMA -- this extends that call site with
 * the update of diffusers' EMAModel, its `s.sub_(omd * (s - p))` form, which Diffusion Policy evaluates on).  THE EMA CONTRACT (identical in
 * csrc/ema.hip and in the numpy restatement tests/ema_reference.py), with s = shadow[i] and omd = one_minus_decay:
 *     shadow[i] = s - omd * (s - float(param[i]))                      i in [0, n)
 *   arithmetic  three fp32 operations -- subtract, multiply, subtract -- each rounded on its own (no FMA contraction).  A bf16 parameter is
 *               widened exactly (its 16 bits become the upper half of the fp32).  omd = 0 keeps a shadow whose difference to the parameter is finite; omd = 1 gives
 *               s - (s - p), the parameter up to the rounding of the difference.
 *   purity      the result is a pure function of (shadow[i], param[i], omd): nothing depends on n, on launch geometry or on which lane holds
 *               the element.  The body moves 16 bytes per lane and instruction, the last n % 8 (bf16) or n % 4 (fp32) elements one per lane.
 *   memory      param is never written; exactly shadow[0 .. n) is written.  Stream-ordered and capturable, no atomics, no workspace.
 *   refusals    OVLA_EINVAL before any launch: a null pointer, n < 0, param or shadow not 16-byte aligned, one_minus_decay outside [0, 1] or
 *               NaN.  n == 0 is legal and launches nothing.
 * The decay schedule (warm-up) is the caller's: vla_scripts/finetune.py `ema_decay_at`. */
typedef struct {
  const void* param;      /* bf16 or fp32 [n] (is_bf16) */
  float* shadow;          /* fp32 [n], in/out */
  int64_t n; int32_t is_bf16;
  float one_minus_decay;  /* in [0, 1] */
} ovla_ema_update_args;
int ovla_ema_update(const ovla_ema_update_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Gradient-norm clipping and the non-finite step guard: torch.nn.utils.clip_grad_norm_(trainable_params, max_norm) in front of the optimizer
 * step (the reference's own loop, vla-scripts/finetune.py:952-1100, never clips; its family -- the native Prismatic trainer's max_grad_norm --
 * does), plus a guard the reference lacks: a step whose gradient norm is NaN or Inf changes nothing.  Three kernels, all stream-ordered and
 * capturable; the norm is complete at a kernel boundary: no atomics, no grid barrier, no spin-wait, no cooperative launch, and no host value
 * depends on the data.  THE CLIP CONTRACT (identical in csrc/grad_clip.hip and in the numpy restatement tests/grad_clip_reference.py):
 *
 * ovla_grad_sumsq: slots[slot] = sum over i in [0, n) of q_i, in double, where
 *     r_i = grad[i] * grad_scale               one fp32 multiply; for a bf16 parameter buffer (is_bf16) rounded to bf16 (RNE) after it:
 *                                              the gradient exactly as ovla_adamw forms it
 *     q_i = (double)r_i * (double)r_i          exact (48 significant bits)
 *   order       FIXED.  Chunk c covers elements [c C, min(n, (c + 1) C)), C = OVLA_GRAD_SUMSQ_CHUNK, and is reduced by one workgroup of
 *               L = OVLA_GRAD_SUMSQ_LANES lanes.  Element c C + o belongs to lane (o / 4) % L; a lane starts at 0.0 and adds its q in ascending
 *               o (trip k = o / (4 L) outermost, then the four elements of its 16-byte group).  The L lane sums s[0 .. L) are paired by THE TREE:
 *               within each run of 64 consecutive lanes, for h = 32, 16, 8, 4, 2, 1: s[t] += s[t + h] for t < h; then the four run totals
 *               w0 .. w3 give (w0 + w1) + (w2 + w3).  The chunk's partial is stored as a double in workspace[c].  A second launch of one
 *               workgroup sums the P = ceil(n / C) partials: lane t starts at 0.0 and adds workspace[t], workspace[t + L], ... in ascending
 *               index, then THE TREE again.  Every addition is a double addition rounded to nearest.
 *   purity      a pure function of (grad[0 .. n), n, grad_scale, is_bf16): nothing depends on the grid, on the workspace's or the slots'
 *               previous contents or on which hardware lane holds an element.  Full 16-byte groups are loaded 16 bytes per lane, the last
 *               n % 4 elements one by one by the lane that owns their group.
 *   memory      reads exactly grad[0 .. n); writes workspace[0 .. P) and slots[slot], nothing else.
 *   refusals    OVLA_EINVAL before any launch: a null pointer, n < 0, slot < 0, grad not 16-byte aligned, slots or workspace not 8-byte
 *               aligned, workspace_bytes < 8 P.  n == 0 is legal and writes 0.0. */
#define OVLA_GRAD_SUMSQ_CHUNK 8192
#define OVLA_GRAD_SUMSQ_LANES 256
typedef struct {
  const float* grad;        /* fp32 [n] */
  int64_t n; int32_t is_bf16;
  float grad_scale;
  double* slots; int32_t slot;
  double* workspace; int64_t workspace_bytes;   /* >= 8 * ceil(n / OVLA_GRAD_SUMSQ_CHUNK) */
} ovla_grad_sumsq_args;
int ovla_grad_sumsq(const ovla_grad_sumsq_args* a, void* stream);

/* ovla_grad_clip_coef: one launch, one lane, ordinary stores.  total = slots[0] + slots[1] + ... + slots[n_slots - 1] in index order, in
 * double, starting from 0.0; state->n_steps += 1; then
 *   total not finite and skip_nonfinite:   skip = 1, coef = 1, norm = (float)sqrt(total) (NaN or Inf as computed), n_skipped += 1
 *   otherwise:                             skip = 0, norm = (float)sqrt(total),
 *                                          coef = fminf(1.f, max_norm / (norm + 1e-6f)) in fp32 (clip_grad_norm_'s formula; a NaN quotient
 *                                          gives 1 by fminf), n_clipped += 1 if coef < 1
 * max_norm = +inf is legal ("guard only": coef is 1 for every finite norm).  OVLA_EINVAL before the launch: a null pointer, n_slots < 1,
 * max_norm <= 0 or NaN.  The state is device memory the caller zeroes once; only this kernel writes it. */
typedef struct { float coef; float norm; int32_t skip; int32_t n_steps, n_clipped, n_skipped; } ovla_grad_clip_state;
typedef struct {
  const double* slots; int32_t n_slots;
  float max_norm;
  int32_t skip_nonfinite;
  void* state;              /* device ovla_grad_clip_state, in/out */
} ovla_grad_clip_coef_args;
int ovla_grad_clip_coef(const ovla_grad_clip_coef_args* a, void* stream);

/* ovla_adamw_clipped: ovla_adamw behind the clip state.  Every workgroup reads state->skip and returns at once when it is set: param,
 * exp_avg and exp_avg_sq keep their bits.  Otherwise the gradient entering the update is
 *     bf16:  bfround(bfround(grad[i] * grad_scale) * coef)        fp32:  (grad[i] * grad_scale) * coef
 * (what grad.mul_(clip_coef) leaves in a .grad of the parameter's dtype), and from there on the element update IS ovla_adamw's: both
 * kernels call one function (csrc/adamw_elem.h).  With coef == 1.0f the result is bit-identical to ovla_adamw.  The fields before
 * clip_state are those of ovla_adamw_args, with the same meaning and the same refusals; a null clip_state is refused too. */
typedef struct {
  void* param; void* exp_avg; void* exp_avg_sq;
  const float* grad;
  int64_t n; int32_t is_bf16; int32_t step;
  double lr, beta1, beta2, eps, weight_decay;
  float grad_scale;
  const void* clip_state;   /* device ovla_grad_clip_state written by ovla_grad_clip_coef earlier on the stream */
} ovla_adamw_clipped_args;
int ovla_adamw_clipped(const ovla_adamw_clipped_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-tensor statistics: for every trainable tensor of one flat buffer, the sum of squares of its gradient as AdamW sees it and of its
 * parameter, the largest finite |gradient|, the number of non-finite gradient elements and a latch that counts the steps on which there
 * were any -- what names the tensor that carried a NaN when the step guard above only says "skipped" (the reference reports such numbers
 * through W&B; torch would need two tiny launches and a host synchronise per tensor).  Opt-in and read-only: it writes nothing but its own
 * partials and out.  One table-driven launch pair per flat buffer, stream-ordered and capturable; every number is complete at a kernel
 * boundary: no atomics, no grid barrier, no spin-wait, no cooperative launch, ordinary vector stores, and no host value depends on the data.
 * THE STATS CONTRACT (identical in csrc/tensor_stats.hip and in the numpy restatement tests/tensor_stats_reference.py), for segment t =
 * (offset_t, n_t) of the table:
 *     r_i = grad[i] * grad_scale        one fp32 multiply, then rounded to bf16 (RNE) when grad_round_bf16 is set: exactly ovla_grad_sumsq's r_i
 *   grad_sumsq   sum over the segment of (double)r_i * (double)r_i in ovla_grad_sumsq's FIXED order, with the chunks counted from the segment's
 *                own start: chunk j of segment t covers offset_t + [j C, min(n_t, (j + 1) C)), C = OVLA_GRAD_SUMSQ_CHUNK, and is reduced by one
 *                workgroup of L = OVLA_GRAD_SUMSQ_LANES lanes; element offset_t + j C + o belongs to lane (o / 4) % L and is added in ascending
 *                o; the lane sums go through THE TREE of the clip contract; the segment's ceil(n_t / C) partials are summed as
 *                ovla_grad_sumsq's second launch sums its P partials (lane j % L in ascending j, THE TREE again).  A one-entry table {0, n}
 *                therefore gives ovla_grad_sumsq's slot bit for bit.  NaN and Inf propagate.
 *   param_sumsq  the same sum over (double)param[i] * (double)param[i], same ownership and order; a bf16 parameter (param_is_bf16) is widened
 *                exactly, an fp32 one (the fp32 buffer, or the fp32 master of a bf16 buffer) is taken as it is.
 *   grad_absmax  the maximum of |r_i| over the finite r_i; 0 when there is none.
 *   n_nonfinite  the number of r_i that are NaN or +-Inf.
 *   n_bad_steps  in/out: incremented by 1 when n_nonfinite > 0, otherwise kept -- a latch that needs no per-step readback.  The caller
 *                zeroes it once.
 *   purity       a pure function of the segment's elements, the table and the scalars: nothing depends on the grid, on the previous contents
 *                of partials or out (other than n_bad_steps), on the other segments or on which hardware lane holds an element.
 *   memory       reads exactly the segments' elements of grad and param -- the padding between segments is never read -- in 16-byte groups
 *                of four gradients (8 bytes of a bf16 parameter), the last n_t % 4 elements one by one by the lane that owns their group.
 *                Writes partials[0 .. 32 total_chunks) and out[0 .. n_segs), nothing else.  Two launches: one workgroup per chunk, which finds
 *                its segment by a binary search of chunk_start, then one workgroup per segment.
 *   segments     n_t == 0 is legal: zero chunks, an all-zero output, n_bad_steps kept.
 *   the plan     ovla_tensor_stats_plan (host only, no device call) checks the table and writes chunk_start[t] = the number of chunks of the
 *                segments before t, t in [0, n_segs]; chunk_start[n_segs] is total_chunks.  The caller copies segs and chunk_start to the
 *                device once.  The library remembers the (n_segs, total_chunks) pair of every plan made in the process, which is all the
 *                launch can check of a table that lives in device memory.
 *   refusals     OVLA_EINVAL before any launch.  From the plan: a null pointer, n_segs < 1, buffer_n < 0, a negative n or offset, offset % 8
 *                != 0, segments not ascending or overlapping (offset_t < offset_{t-1} + n_{t-1}), a segment past buffer_n, more chunks than
 *                a grid covers.  From the launch: a null pointer, n_segs < 1, total_chunks < 0, grad or param not 16-byte aligned, out, partials or
 *                segs not 8-byte aligned, chunk_start not 4-byte aligned, partials_bytes < OVLA_TENSOR_STATS_PARTIAL_BYTES total_chunks, and a
 *                (n_segs, total_chunks) pair no plan of this process produced (total_chunks different from the plan's). */
#define OVLA_TENSOR_STATS_PARTIAL_BYTES 32
typedef struct { int64_t offset, n; } ovla_tensor_seg;   /* elements of the flat buffer; offset % 8 == 0 */
typedef struct {
  double grad_sumsq, param_sumsq;
  float grad_absmax;
  int32_t n_bad_steps;
  int64_t n_nonfinite;
} ovla_tensor_stat;                                       /* 32 bytes */
int ovla_tensor_stats_plan(const ovla_tensor_seg* segs, int32_t n_segs, int64_t buffer_n, int32_t* chunk_start /* n_segs + 1 */);
typedef struct {
  const float* grad;                /* fp32 flat gradient buffer */
  const void* param;                /* bf16 or fp32 (param_is_bf16) flat parameter buffer, the same element indices */
  int32_t param_is_bf16, grad_round_bf16;
  float grad_scale;
  const ovla_tensor_seg* segs;      /* device [n_segs] */
  const int32_t* chunk_start;       /* device [n_segs + 1] */
  int32_t n_segs, total_chunks;
  void* partials;
  int64_t partials_bytes;           /* >= OVLA_TENSOR_STATS_PARTIAL_BYTES * total_chunks */
  ovla_tensor_stat* out;            /* device [n_segs]; n_bad_steps is in/out, every other field is written */
} ovla_tensor_stats_args;
int ovla_tensor_stats(const ovla_tensor_stats_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * AdamW on fp32 master weights: the optimizer step of a bf16 parameter buffer whose state is kept in fp32 (opt-in,
 * ParamStore.enable_fp32_state; the default stays ovla_adamw's torch-faithful bf16 state).  In bf16, exp_avg_sq.mul_(0.999) returns its
 * input for every normal value (the decrement is below half an ulp: the second moment never decays) and a parameter update below half an
 * ulp of the parameter is lost; here an fp32 master copy and fp32 moments take the update and the bf16 parameter is the rounded master.
 * THE MASTER CONTRACT (identical in csrc/adamw_master.hip and in the restatement tests/adamw_master_reference.py), for i in [0, n):
 *   gradient     r = grad[i] * grad_scale, one fp32 multiply and NO bf16 rounding: the optimizer-side dtype is fp32.  With clip_state,
 *                r = r * state->coef, a second fp32 multiply (ovla_adamw_clipped's fp32 form).  If state->skip is set every workgroup
 *                returns at once: master, exp_avg, exp_avg_sq and param keep their bits.
 *   update       (master[i], exp_avg[i], exp_avg_sq[i]) <- ovla_adamw's fp32 element update of them with gradient r: one function
 *                (csrc/adamw_elem.h adamw_update_f32) is called by both kernels, with the same scalars, no FMA contraction.
 *   publication  param[i] = bf16_rne(master[i]) of the NEW master: NaN stays NaN, a value beyond the largest finite bf16 gives +-Inf, as
 *                torch's .to(bfloat16).  After every call that is not skipped, param == bf16_rne(master) element for element.
 *   purity       each output element is a pure function of (master[i], exp_avg[i], exp_avg_sq[i], grad[i]) and the scalars: nothing
 *                depends on n, on launch geometry or on which lane holds the element.  The body moves four elements per lane and trip
 *                (16-byte loads of grad, master and the moments, 16-byte stores of the three, one 8-byte store of four bf16), the last
 *                n % 4 elements one per lane; a grid-stride loop under OVLA_ADAMW_MASTER_MAX_BLOCKS workgroups of 256 lanes.
 *   memory       grad is never written; exactly [0, n) of master, exp_avg, exp_avg_sq and param is written.  Stream-ordered and
 *                capturable, no atomics, no workspace.  30 bytes per element (16 read, 14 written); ovla_adamw on bf16 moves 16.
 *   refusals     OVLA_EINVAL before any launch: a null pointer other than clip_state, n <= 0, step < 1, or master, exp_avg, exp_avg_sq,
 *                param or grad not 16-byte aligned. */
#define OVLA_ADAMW_MASTER_MAX_BLOCKS 2048
typedef struct {
  float* master; float* exp_avg; float* exp_avg_sq;   /* fp32 [n], in/out */
  void* param;                                        /* bf16 [n], out */
  const float* grad;                                  /* fp32 [n] */
  int64_t n; int32_t step;                            /* step >= 1 (after increment, as torch) */
  double lr, beta1, beta2, eps, weight_decay;
  float grad_scale;
  const void* clip_state;   /* NULL, or a device ovla_grad_clip_state written by ovla_grad_clip_coef earlier on the stream */
} ovla_adamw_master_args;
int ovla_adamw_master(const ovla_adamw_master_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * DDIM sampling on the device (prismatic/extern/hf/modeling_prismatic.py:793-877 `_run_diffusion_prediction`: per step, timestep
 * embedding + noisy actions in, `noise_scheduler.step(noise_pred, t, curr_noisy_actions).prev_sample` out).  The loop's step index k is a
 * DEVICE int32 that both kernels read and ovla_ddim_step advances, so one sampling step has no host-dependent argument and can be replayed
 * from a captured graph; k outside [0, n_steps) makes either kernel a no-op.
 *
 * ovla_ddim_prepare, top of step k: temb[b, :] = temb_table[k, :] for b < B (the timestep token of each observation; temb_table bf16
 * [n_steps, D] is the host's time_encoder(t_k) rounded to bf16) and noisy[i] = bf16(sample[i]), i < n (the noisy-action projector's input). */
typedef struct { const int32_t* step; const void* temb_table; void* temb; const float* sample; void* noisy; int32_t n_steps, B, D, n; } ovla_ddim_prepare_args;
int ovla_ddim_prepare(const ovla_ddim_prepare_args* a, void* stream);
/* ovla_ddim_step, end of step k: diffusers' DDIMScheduler.step for epsilon prediction with clip_sample and eta = 0, then the sampler's
 * bf16 round trip, in place on sample fp32 [n] with eps bf16 [n] (the head's output) and coef fp32 [n_steps, 4], row k =
 * ((1 - a_t)^1/2, a_t^1/2, a_prev^1/2, (1 - a_prev)^1/2) built by the host with the scheduler's own expressions:
 *     x0 = clamp((s - c0 e) / c1, -1, 1);   e' = (s - c1 x0) / c0;   s <- float(bf16(c2 x0 + c3 e'))
 * Every multiply / subtract / divide / add is rounded on its own (no FMA contraction, correctly rounded division): bit-identical to the CPU
 * torch expression.  One workgroup; *step becomes k + 1 once every element has been written. */
typedef struct { float* sample; const void* eps; const float* coef; int32_t* step; int32_t n_steps, n; } ovla_ddim_step_args;
int ovla_ddim_step(const ovla_ddim_step_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Diffusion noise (DiffusionActionHead.sample_noisy_actions, prismatic/models/action_heads.py:167-197: per training batch N(0, 1) noise of
 * the chunk's shape, one uniform timestep per sample, noise_scheduler.add_noise, the sinusoidal timestep embedding).  ONE launch draws all
 * four for B samples of n = chunk * action_dim elements; nothing comes from or goes to the host, and the position of the stream is the
 * 32-bit `call` the caller advances once per draw and checkpoints.  THE NOISE CONTRACT (identical in csrc/diffusion_noise.hip and in the
 * numpy restatement tests/diffusion_noise_reference.py); every output is a pure function of (seed, call, stream, sample b, element i):
 *   generator   Philox4x32-10 as in "LoRA dropout" above: counter (c0, c1, c2, c3), key (seed_lo, seed_hi).
 *   streams     c2 = stream: 0 training noise, 1 the timestep draw, 2 the sampler's start noise.  The `stream` argument selects the NOISE stream
 *               and must be 0 or 2; 1 is refused (the timestep draw always uses it), so is every other value.
 *   timestep    o = philox(0, b, 1, call);  t_b = umulhi(o[0], T) = floor(o[0] * T / 2^32) in [0, T);  timesteps[b] = t_b.
 *   embedding   temb[b, :] = temb_table[t_b, :], an exact copy (temb_table bf16 [T, D] contiguous: the host's time encoder of float(t) rounded
 *               to bf16, row by row).
 *   noise       elements 4 j .. 4 j + 3 of sample b come from o = philox(j, b, stream, call): two Box-Muller pairs in fp32,
 *               (o[0], o[1]) -> elements 4 j, 4 j + 1 and (o[2], o[3]) -> 4 j + 2, 4 j + 3.  For a pair (w_a, w_b):
 *                   u1 = ((w_a >> 8) + 1) * 2^-24 in (0, 1],   u2 = (w_b >> 8) * 2^-24 in [0, 1)        (both exact in fp32)
 *                   r = sqrtf(-2 logf(u1)),   z_even = r * cos(2 pi u2),   z_odd = r * sin(2 pi u2)
 *               with cos / sin of 2 pi u2 evaluated as sincospif(2 u2) (exact argument reduction).  |z| <= sqrt(48 ln 2) = 5.77.
 *               noise[b, i] = bf16_rne(z_i).  A tail (n % 4 != 0) discards the unused values of the last call.
 *   noisy       noisy[b, i] = bf16_rne(ab[t_b][0] * float(actions[b, i]) + ab[t_b][1] * float(noise[b, i])): add_noise in fp32 on the bf16-rounded
 *               noise, two multiplies and one add each rounded on its own (no FMA contraction).  ab fp32 [T, 2] contiguous, row t =
 *               (alphas_cumprod[t]^1/2, (1 - alphas_cumprod[t])^1/2) built by the host with the scheduler's own expressions.
 *   indexing    b and i are the logical sample and element; nothing depends on B, on a row stride or on launch geometry.
 * actions / noise / noisy bf16 [B, n] and temb bf16 [B, D] each with its own row stride in elements (>= n, >= D; elements past a row's
 * extent are neither read nor written); timesteps int32 [B].  Stream-ordered and capturable, no atomics, no workspace; launches nothing on
 * OVLA_EINVAL. */
typedef struct {
  const void* actions; int64_t ld_actions;
  const float* ab;                   /* fp32 [T, 2] */
  const void* temb_table;            /* bf16 [T, D] */
  void* noise; int64_t ld_noise;
  void* noisy; int64_t ld_noisy;
  void* temb; int64_t ld_temb;
  int32_t* timesteps;
  uint32_t seed_lo, seed_hi, call, stream;
  int32_t B, n, D, T;
} ovla_diffusion_noise_args;
int ovla_diffusion_noise(const ovla_diffusion_noise_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Token sampling and the policy-gradient objective (the discrete action-token path beyond greedy decode and cross entropy: draw the chunk's
 * tokens from the tempered softmax over a token window, report their log-probabilities and entropy, and the gradient of the PPO / GRPO
 * clipped surrogate).  Everything stays on the device; the position of the random stream is the 32-bit `call` the caller advances once per
 * draw and checkpoints.  One workgroup of 256 lanes per row, always: a row's bits depend on neither the row count nor the row's position.
 * The row reductions are csrc/token_row.h, the body ovla_token_ce is built from.  THE SAMPLING CONTRACT (identical in csrc/token_sample.hip
 * and in the numpy restatement tests/token_sample_reference.py), for one row z[0 .. vocab) of bf16 logits, window [lo, hi), temperature T:
 *   scale       invT = 1.0f / T (IEEE division);  s_j = float(z_j) * invT, one rounded fp32 multiply (no FMA contraction anywhere below).
 *   generator   Philox4x32-10 as in "LoRA dropout" above.  Token id j (ABSOLUTE, not relative to the window) takes word w = o[j & 3] of
 *               o = philox(j >> 2, row_key, 3, call) with key (seed_lo, seed_hi).  row_key is row_key[r], or r itself without the array.
 *   uniform     u = float(2 (w >> 9) + 1) * 2^-24: exact in fp32, strictly inside (0, 1), symmetric about 1/2.
 *   Gumbel      g = -logf(-logf(u)) with the accurate logf (the winners have u near 1, where -log u is tiny and a fast log's absolute
 *               error would dominate).  g lies in [-2.812, 16.636].
 *   draw        key_j = s_j + g;  token = the LOWEST index of the maximum key over the window (Gumbel-max: P(token = j) = softmax(s)_j).
 *               A NaN key never wins; -inf inside the window has probability 0 and is never drawn.
 *   logprob     lse = __logf(sum_j __expf(s_j - m)) + m over the window, m = max_j s_j, in token_row.h's order (lane t sums j = lo + t,
 *               lo + t + 256, ...; wave butterfly; (w0 + w1) + (w2 + w3));  logprob = s_token - lse.
 *   entropy     lse - (sum_j e_j s_j) / (sum_j e_j), e_j = __expf(s_j - m), a term with e_j == 0 skipped, the numerator in the same order.
 *   degenerate  a window whose maximum is not finite (all -inf; or a +inf): token = lo, logprob = entropy = NaN.
 *   isolation   columns outside [lo, hi) influence nothing, whatever they hold; columns >= vocab are never read.
 *   bin         clip(n_tokens - token - 1, 0, n_bins - 1), ovla_argmax_bins' rule.
 * state_dev (optional, DEVICE uint32[3] = seed_lo, seed_hi, call) overrides the three host values when the kernel runs, so a captured graph
 * draws fresh values on every replay.  With a 16-byte aligned base and ld % 8 == 0 the key pass loads whole 8-column groups as 16 bytes and
 * does the head and the tail of the window column by column.  logits bf16 [rows, ld]; token / bin int32 [rows]; logprob / entropy fp32
 * [rows] (entropy optional); row_key int32 [rows] (optional).
 *
 * ovla_token_pg: for GIVEN tokens (clamped into the window), in one launch, the same logprob and entropy and
 *   ratio   = expf(logprob - old_logprob[r])     (accurate expf), or exactly 1 without old_logprob
 *   gate    = 0 if (adv >= 0 and ratio > clip_hi) or (adv < 0 and ratio < clip_lo), otherwise ratio;   clipped[r] = (gate == 0)
 *   c       = ((adv[r] * gate) * grad_scale) * invT
 *   dlogits[r, j] = bf16(fmaf(e_j, 1.0f / sum, -[j == token]) * c) for j in the window, +0 for every other j < vocab   (optional; may alias logits)
 * the gradient of -sum_r min(ratio A, clip(ratio, clip_lo, clip_hi) A) * grad_scale.  A gated row is STORED as zeros, never multiplied
 * through (ovla_lora_route's convention).  With T = 1, the window [0, vocab), no old_logprob, adv = 1: dlogits and -logprob are
 * ovla_token_ce's dlogits and loss_rows bit for bit.  advantage / old_logprob fp32 [rows] on the device; tokens int32 [rows].
 *
 * Both are stream-ordered and capturable, use no atomics and no workspace, and launch nothing on OVLA_EINVAL: a null pointer, rows or vocab
 * <= 0, ld < vocab, a window that is empty or leaves [0, vocab], T <= 0 or NaN or inf, clip_lo > clip_hi or a NaN bound.
 *
 * THE GROUP FORMS (GRPO: G draws per observation from one forward; 1 <= G <= OVLA_PG_GROUP_MAX).
 * ovla_sample_tokens_group: token / bin / logprob int32 / int32 / fp32 [rows, G], entropy fp32 [rows] (optional), row_key int32 [rows, G]
 * (optional; without it the key of draw (r, g) is r * G + g).  Draw (r, g) is, bit for bit, what ovla_sample_tokens returns for logits row r
 * under row key row_key[r, g], and entropy[r] is that kernel's entropy: it is the same kernel, one workgroup per (r, g).
 *
 * ovla_token_pg_group: G GIVEN samples per row in one launch, one workgroup per row.  tokens int32 / advantage fp32 [rows, G]; old_logprob /
 * ref_logprob fp32 [rows, G] (optional); logprob / ratio fp32, clipped int32 [rows, G]; kl fp32 [rows, G], given exactly when ref_logprob is;
 * entropy fp32 [rows]; dlogits bf16 [rows, ld_d] (optional; may alias logits).  The gradient with respect to the logits of
 *   sum_{r,g} [ -min(ratio A, clip(ratio) A) + kl_coef * kl ]_{r,g} * grad_scale  -  ent_scale * sum_r H_r
 * With m, sum, lse and H = entropy from token_row.h exactly as in ovla_token_pg, per sample g (each line one rounded fp32 operation per
 * operator, left to right as bracketed, no FMA contraction):
 *   logprob_g = s_tok_g - lse;  ratio_g, gate_g, clipped_g as in ovla_token_pg
 *   c_g   = ((adv_g * gate_g) * grad_scale) * invT, and +0 (set, not multiplied) for a gated sample and for adv_g == 0 (a padding sample,
 *           whatever its old_logprob holds)
 *   with ref_logprob:  d_g = ref_g - logprob_g;  x_g = expm1f(d_g) (accurate);  kl_g = x_g - d_g  (Schulman's k3: exactly +0 on policy, >= 0);
 *                      k_g = ((kl_coef * x_g) * grad_scale) * invT;  w_g = c_g + k_g.  The KL term is not gated.
 *   without:           w_g = c_g (no add)
 *   a sample with w_g == 0 is SKIPPED, never multiplied through (a NaN elsewhere in the row cannot leak in through it).
 * Per column j of the window, e_j = __expf(s_j - m), inv = 1.0f / sum:
 *   acc = t_{g1} + t_{g2} + ... in ascending g over the samples not skipped, t_g = fmaf(e_j, inv, -[j == token_g]) * w_g, the first term
 *         taken as it is, each further term one rounded fp32 add;  acc = +0 when every sample is skipped
 *   if ent_scale != 0 and e_j > 0:  acc = acc + ((ent_scale * invT) * (e_j * inv)) * ((s_j - lse) + H), added last
 *   dlogits[r, j] = bf16(acc);  +0 for every j < vocab outside the window;  columns >= vocab are never touched.
 * A row with every sample skipped and ent_scale == 0 is STORED as +0 on [0, vocab).  All G values s_tok_g are read, and a barrier passed,
 * before any lane stores.  With G = 1, no ref_logprob, ent_scale == 0 and adv != 0: ovla_token_pg's outputs bit for bit.
 * Refusals (OVLA_EINVAL, nothing launched): ovla_token_pg's / ovla_sample_tokens'; G outside [1, OVLA_PG_GROUP_MAX]; kl_coef negative or
 * NaN; ent_scale NaN; ref_logprob without kl or kl without ref_logprob. */
#define OVLA_PG_GROUP_MAX 64
typedef struct {
  const void* logits; int64_t ld;
  int32_t* token; int32_t* bin; float* logprob; float* entropy;
  const uint32_t* state_dev; const int32_t* row_key;
  uint32_t seed_lo, seed_hi, call;
  float temperature;
  int32_t rows, vocab, lo, hi, n_tokens, n_bins, G;
} ovla_sample_tokens_group_args;
int ovla_sample_tokens_group(const ovla_sample_tokens_group_args* a, void* stream);

typedef struct {
  const void* logits; int64_t ld;
  const int32_t* tokens; const float* advantage; const float* old_logprob; const float* ref_logprob;
  float* logprob; float* ratio; int32_t* clipped; float* kl; float* entropy;
  void* dlogits; int64_t ld_d;
  float temperature, clip_lo, clip_hi, grad_scale, kl_coef, ent_scale;
  int32_t rows, G, vocab, lo, hi;
} ovla_token_pg_group_args;
int ovla_token_pg_group(const ovla_token_pg_group_args* a, void* stream);

typedef struct {
  const void* logits; int64_t ld;
  int32_t* token; int32_t* bin; float* logprob; float* entropy;
  const uint32_t* state_dev; const int32_t* row_key;
  uint32_t seed_lo, seed_hi, call;
  float temperature;
  int32_t rows, vocab, lo, hi, n_tokens, n_bins;
} ovla_sample_tokens_args;
int ovla_sample_tokens(const ovla_sample_tokens_args* a, void* stream);

typedef struct {
  const void* logits; int64_t ld;
  const int32_t* tokens; const float* advantage; const float* old_logprob;
  float* logprob; float* entropy; float* ratio; int32_t* clipped;
  void* dlogits; int64_t ld_d;
  float temperature, clip_lo, clip_hi, grad_scale;
  int32_t rows, vocab, lo, hi;
} ovla_token_pg_args;
int ovla_token_pg(const ovla_token_pg_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Laplace policy on the L1 head (the continuous path beyond regression: L1 regression is maximum likelihood for a Laplace distribution of
 * fixed scale b around the head's prediction mu, so that distribution is the policy the L1 head already is -- the modes coincide and the L1
 * loss gradient is the policy's score up to 1 / b).  ovla_laplace_sample draws G chunks per row around mu and reports their log-probabilities;
 * ovla_laplace_pg computes, for GIVEN draws, the same log-probabilities, the PPO / GRPO clipped surrogate, the closed-form KL to a reference
 * prediction of the same scale, and their gradient with respect to mu: the `dpred` ovla_head_out_bwd takes.  The forward does not depend on the
 * draws, so G draws per observation share one forward and one backward.  Everything stays on the device; the generator is the token
 * sampler's (seed, `call` advanced once per draw by the caller) on a stream word of its own.
 * Shared conventions: pred (mu) bf16 [rows, adim], rows = B * chunk, what ovla_head_out_fwd stores; 1 <= adim <= 16; 1 <= G <= OVLA_PG_GROUP_MAX;
 * scale[d] = b_d > 0 and finite, log_norm[d] = float32(log(2 b_d)) formed by the caller in double (no logf enters the log-probability), both by
 * value, entries >= adim ignored; inv_b_d = 1.0f / b_d (IEEE division).  Every operator below is one rounded fp32 operation in the bracketing
 * written, no FMA contraction.  THE CONTRACT (identical in csrc/laplace_policy.hip and in the numpy restatement
 * tests/laplace_policy_reference.py):
 *   logprob     q_d = fabsf(a_d - mu_d) * inv_b_d;  acc = 0;  acc = acc - (q_d + log_norm[d]) for ascending d;  logprob = acc.
 *
 * ovla_laplace_sample: action fp32 [rows, G, adim], logprob fp32 [rows, G]; row_key int32 [rows, G] (optional; without it the key of draw
 * (r, g) is r * G + g).  For dimension d of the draw with key `key`:
 *   generator   Philox4x32-10 as in "LoRA dropout" above: word w = o[d & 3] of o = philox(d >> 2, key, 4, call) with key (seed_lo, seed_hi).
 *               (Stream word 4: the token sampler uses 3 on the same seed.)
 *   uniform     u = float(2 (w >> 9) + 1) * 2^-24: exact in fp32, strictly inside (0, 1), symmetric about 1/2.
 *   variate     x = u - 0.5f;  t = 1.0f - 2.0f * fabsf(x): both exact, x != 0, t in [2^-23, 1 - 2^-23];  the variate is exactly symmetric.
 *   noise       e = copysignf(-logf(t), x) with the accurate logf: a unit Laplace variate (E|e| = 1, E e^2 = 2), |e| <= 15.943.
 *   action      a_d = mu_d + b_d * e, stored;  the log-probability is computed from the STORED a_d, not from e: the bits ovla_laplace_pg
 *               recomputes from the stored draw.
 * state_dev (optional, DEVICE uint32[3] = seed_lo, seed_hi, call) overrides the three host values when the kernel runs, as in ovla_sample_tokens.
 *
 * ovla_laplace_pg: G GIVEN samples per row in one launch, one workgroup of 64 lanes per row.  actions fp32 [rows, G, adim]; advantage fp32
 * [rows, G]; old_logprob fp32 [rows, G] (optional); ref_pred bf16 [rows, adim] (optional: the KL term exists exactly when it is given);
 * logprob / ratio fp32, clipped int32 [rows, G]; kl fp32 [rows], given exactly when ref_pred is; dpred bf16 [rows, adim] (optional).
 * Per sample g:
 *   logprob_g as above;  ratio_g = expf(logprob_g - old_g) (accurate expf), or exactly 1 without old_logprob
 *   gate_g, clipped_g by ovla_token_pg's rule;  c_g = (adv_g * gate_g) * grad_scale, and +0 (set, not multiplied) for a gated sample and for
 *   adv_g == 0.  A sample with c_g == 0 is SKIPPED, never multiplied through, and its actions are not read for the gradient: a padding draw
 *   full of NaN cannot leak into the row.
 * Per (r, d):
 *   acc = t_{g1,d} + t_{g2,d} + ... in ascending g over the samples not skipped, t_{g,d} = (sgn(mu_d - a_{g,d}) * inv_b_d) * c_g with
 *         sgn(0) = 0 (taken from comparisons: a NaN action gives 0), the first term taken as it is, each further term one rounded fp32 add;
 *         acc = +0 when every sample is skipped
 *   with ref_pred:  D = mu_d - ref_d;  q = fabsf(D) * inv_b_d;  x = -expm1f(-q) (accurate expm1f);  kl_d = q - x, which is
 *         KL(Laplace(mu, b) || Laplace(ref, b)) of the dimension, exactly +0 on policy and >= 0;  kl[r] = kl_0 + kl_1 + ... in ascending d;
 *         k_d = ((kl_coef * x) * kl_scale) * (sgn(D) * inv_b_d);  acc = acc + k_d, added last.  The KL term is not gated.
 *   dpred[r, d] = bf16(acc)
 * the gradient with respect to mu of  sum_{r,g} -min(ratio A, clip(ratio) A) * grad_scale  +  kl_coef * kl_scale * sum_r kl[r].  With G = 1,
 * adv = 1, b = 1, no old_logprob and no ref_pred: dpred = bf16(sgn(mu - a) * grad_scale), the bits ovla_head_out_bwd forms for the L1 loss.
 *
 * Both are stream-ordered and capturable, use no atomics and no workspace; a row's bits depend on its inputs and its row keys only, never on
 * `rows` or the row's position.  Refusals (OVLA_EINVAL, nothing launched): a null required pointer; rows <= 0; adim outside [1, 16]; G outside
 * [1, OVLA_PG_GROUP_MAX]; a scale that is not positive and finite; clip_lo > clip_hi or a NaN bound; kl_coef negative or NaN; ref_pred
 * without kl or kl without ref_pred. */
typedef struct {
  const void* pred;
  float* action; float* logprob;
  const uint32_t* state_dev; const int32_t* row_key;
  uint32_t seed_lo, seed_hi, call;
  float scale[16], log_norm[16];
  int32_t rows, adim, G;
} ovla_laplace_sample_args;
int ovla_laplace_sample(const ovla_laplace_sample_args* a, void* stream);

typedef struct {
  const void* pred; const void* ref_pred;
  const float* actions; const float* advantage; const float* old_logprob;
  float* logprob; float* ratio; int32_t* clipped; float* kl;
  void* dpred;
  float scale[16], log_norm[16];
  float clip_lo, clip_hi, grad_scale, kl_coef, kl_scale;
  int32_t rows, adim, G;
} ovla_laplace_pg_args;
int ovla_laplace_pg(const ovla_laplace_pg_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Laplace policy with a learned scale (the fixed-scale pair above with the scale per chunk step and action dimension: a scale head predicts
 * s = log b beside the L1 head's mu; maximum likelihood fits it on demonstrations, the policy gradient moves mu and s together, the
 * closed-form KL to a frozen reference of its own scale and an entropy bonus keep it in place).  ovla_laplace_sample_rows is
 * ovla_laplace_sample with the scale per element; ovla_laplace_pg_rows is ovla_laplace_pg with the scale per element, the gradient with
 * respect to s, the KL between two Laplace distributions of different scale, and the entropy.  Everything of "Laplace policy on the L1 head"
 * carries over: pred bf16 [rows, adim], 1 <= adim <= 16, 1 <= G <= OVLA_PG_GROUP_MAX; stream-ordered, capturable, no atomics, no workspace;
 * every operator one rounded fp32 operation in the bracketing written, no FMA contraction; a row's bits depend on its own inputs and keys
 * only.  THE CONTRACT (identical in csrc/laplace_scale.hip and in the numpy restatement tests/laplace_scale_reference.py):
 * log_scale (s) bf16 [rows, adim], the scale head's raw output; s_lo <= s_hi finite floats by value.  Per element
 *   s_c      = fminf(fmaxf(s, s_lo), s_hi)            (a NaN s acts as s_lo)
 *   inside   = (s >= s_lo && s <= s_hi)               (false for NaN)
 *   b        = expf(s_c) (accurate expf);  inv_b = 1.0f / b (IEEE division);  log_norm = s_c + LN2F, LN2F = float32(ln 2) = 0x1.62e43p-1f
 * Where s_c == 0: b = inv_b = 1, log_norm = LN2F -- what the fixed-scale kernels are handed for scale 1.
 *
 * ovla_laplace_sample_rows: generator, uniform, variate, noise, state_dev and the default keys r * G + g exactly as ovla_laplace_sample (the
 * SAME stream word 4: the same noise at another width).  a_d = mu_d + b_{r,d} * e, stored;  logprob: acc = 0;  acc = acc - (fabsf(a_d - mu_d)
 * * inv_b + log_norm) for ascending d, from the STORED a_d.  entropy fp32 [rows] (optional): the entropy below, stored by the row's draw
 * g = 0.  With log_scale == 0 everywhere: ovla_laplace_sample's bits at scale 1.
 *
 * ovla_laplace_pg_rows: G GIVEN samples per row, one workgroup of 64 lanes per row.  Inputs as ovla_laplace_pg, and log_scale; ref_pred
 * and ref_log_scale bf16 [rows, adim] and the output kl fp32 [rows] come all three or not at all.  Outputs logprob / ratio fp32, clipped
 * int32 [rows, G]; entropy fp32 [rows] (always); dpred, dlog_scale bf16 [rows, adim] (each optional, independently).
 * Per sample g: logprob_g as above; ratio_g, gate_g, clipped_g and c_g = (adv_g * gate_g) * grad_scale by ovla_laplace_pg's rules: c_g is
 * +0 (set, not multiplied) for a gated sample and for adv_g == 0, such a sample is SKIPPED and its actions are not read for any gradient.
 * Per (r, d), with q_g = fabsf(a_{g,d} - mu_d) * inv_b, over the samples not skipped in ascending g, the first term taken as it is, each
 * further term one rounded fp32 add, +0 when every sample is skipped:
 *   acc_mu = sum of (sgn(mu_d - a_{g,d}) * inv_b) * c_g                                  (ovla_laplace_pg's sum)
 *   acc_s  = sum of (1.0f - q_g) * c_g                                                   (d(-c logprob)/ds: d logprob / d s = q - 1)
 * with a reference (s_rc: ref_log_scale clamped by the same bounds):
 *   u = s_c - s_rc;  D = mu_d - ref_d;  q = fabsf(D) * inv_b;  x = -expm1f(-q);  rho = expf(u)      (accurate expm1f, expf)
 *   kl_d   = (expm1f(u) - u) + rho * (q - x)         KL(Laplace(mu, b) || Laplace(ref, b_ref)) of the dimension;  kl[r] = kl_0 + kl_1 + ...
 *   acc_mu = acc_mu + (((kl_coef * x) * kl_scale) * (sgn(D) * inv_b)) * rho              (d kl_d / d mu = sgn(D) x inv_b rho)
 *   acc_s  = acc_s + (kl_coef * kl_scale) * (((rho * (1.0f - x)) * (1.0f + q)) - 1.0f)   (d kl_d / d s = rho (1 - x)(1 + q) - 1)
 *   added after the sample sum and not gated.  At equal scales (u = 0, rho = 1) kl_d and the mean's term are ovla_laplace_pg's bits; on
 *   policy (u = 0, D = 0) kl_d and both gradient terms are exactly +0.
 * entropy[r] = (1.0f + log_norm_0) + (1.0f + log_norm_1) + ... in ascending d (the Laplace entropy; it does not depend on mu); the loss
 * carries -entropy_coef * ent_scale * entropy[r]:
 *   if entropy_coef != 0:  acc_s = acc_s - (entropy_coef * ent_scale), last.
 * dpred[r, d] = bf16(acc_mu);  dlog_scale[r, d] = inside ? bf16(acc_s) : +0  (a clamped or NaN log-scale takes no gradient from any term).
 * The gradient with respect to (mu, s) of  sum_{r,g} -min(ratio A, clip(ratio) A) * grad_scale  +  kl_coef * kl_scale * sum_r kl[r]
 * - entropy_coef * ent_scale * sum_r entropy[r].  With G = 1, adv = 1, no old_logprob, no reference and entropy_coef = 0 it is the gradient
 * of the Laplace negative log-likelihood of a target chunk: dlog_scale = bf16((1 - q) * grad_scale), dpred the L1 gradient divided by b.
 * Refusals (OVLA_EINVAL, nothing launched): those of the fixed-scale pair; a null log_scale; s_lo > s_hi or a bound that is not finite;
 * ref_pred / ref_log_scale / kl not all given or all absent; a null entropy (ovla_laplace_pg_rows); entropy_coef negative or NaN. */
typedef struct {
  const void* pred; const void* log_scale;
  float* action; float* logprob; float* entropy;
  const uint32_t* state_dev; const int32_t* row_key;
  uint32_t seed_lo, seed_hi, call;
  float s_lo, s_hi;
  int32_t rows, adim, G;
} ovla_laplace_sample_rows_args;
int ovla_laplace_sample_rows(const ovla_laplace_sample_rows_args* a, void* stream);

typedef struct {
  const void* pred; const void* log_scale; const void* ref_pred; const void* ref_log_scale;
  const float* actions; const float* advantage; const float* old_logprob;
  float* logprob; float* ratio; int32_t* clipped; float* kl; float* entropy;
  void* dpred; void* dlog_scale;
  float s_lo, s_hi, clip_lo, clip_hi, grad_scale, kl_coef, kl_scale, entropy_coef, ent_scale;
  int32_t rows, adim, G;
} ovla_laplace_pg_rows_args;
int ovla_laplace_pg_rows(const ovla_laplace_pg_rows_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Preference optimisation on the Laplace policy (DPO / IPO on the L1 head: supervision by comparisons instead of rewards.  Per observation
 * a CHOSEN and a REJECTED chunk and a reference prediction; the loss is a function of one scalar, the margin m between the two chunks'
 * summed log-ratios to the reference, and its gradient with respect to the prediction is the group policy gradient of the pair -- the
 * chosen chunk with advantage +k, the rejected one with -k, k out of m).  ovla_laplace_dpo reduces m over an observation's chunk steps,
 * forms k and applies it in ONE launch: dpred / dlog_scale are what ovla_head_out_bwd takes, so a preference step is one training forward
 * and one backward.  Conventions of the two sections above: stream-ordered, capturable, no atomics, no workspace; every operator one rounded
 * fp32 operation in the bracketing written, no FMA contraction; an observation's bits depend on its own inputs only, never on B or on its
 * position.  THE CONTRACT (identical in csrc/laplace_dpo.hip and in the numpy restatement tests/laplace_dpo_reference.py):
 * One workgroup of 64 lanes per observation b, which owns rows b * chunk .. b * chunk + chunk - 1;  rows = B * chunk;
 * 1 <= chunk <= OVLA_DPO_CHUNK_MAX;  1 <= adim <= 16.  pred, ref_pred bf16 [rows, adim];  chosen, rejected fp32 [rows, adim] (RAW chunks);
 * weight fp32 [B] (optional, default 1; must be >= 0).  The scale is EITHER scale[16] / log_norm[16] by value, as ovla_laplace_pg takes them
 * (both policies share it), OR log_scale and ref_log_scale bf16 [rows, adim] with s_lo / s_hi, each element by ovla_laplace_pg_rows' rules
 * (s_c, inside, b = expf(s_c), inv_b = 1.0f / b, log_norm = s_c + LN2F); the two pointers come together and select this form.
 * Per chunk step c (row r = b * chunk + c), by the body  acc = 0;  acc = acc - (fabsf(a_d - mu_d) * inv_b_d + log_norm_d), ascending d:
 *   lp_w[c], lp_l[c]     the chosen and the rejected chunk under (pred, scale)
 *   rlp_w[c], rlp_l[c]   the same two under (ref_pred, the reference's scale)
 *   logprob[r] = (lp_w, lp_l), ref_logprob[r] = (rlp_w, rlp_l), fp32 [rows, 2] (each optional): the bits ovla_laplace_pg /
 *   ovla_laplace_pg_rows reports for the same chunk on pred and on ref_pred.
 * Per observation:
 *   h_w = (lp_w[0] - rlp_w[0]) + (lp_w[1] - rlp_w[1]) + ... in ascending c, the first term taken as it is, each further term one rounded add;
 *   h_l the same of the rejected chunk;  m = h_w - h_l.    h[b] = (h_w, h_l) fp32 [B, 2];  margin[b] = m.
 *   loss_type 0 (sigmoid, eps = label_smoothing):  z = beta * m;  az = fabsf(z);  e = expf(-az) (accurate expf; in (0, 1] at any |z|);
 *     den = 1.0f + e;  l = logf(den) (accurate logf);  s_big = 1.0f / den;  s_small = e / den  (IEEE divisions)
 *     softplus(-z) = (z < 0 ? az : 0.0f) + l;   softplus(z) = (z > 0 ? az : 0.0f) + l
 *     sigma(-z) = z >= 0 ? s_small : s_big;     sigma(z) = z >= 0 ? s_big : s_small;     one_m = 1.0f - eps
 *     loss_b = (one_m * softplus(-z)) + (eps * softplus(z));     k = ((one_m * sigma(-z)) - (eps * sigma(z))) * beta
 *   loss_type 1 (IPO):  tau = 1.0f / (2.0f * beta);  dm = m - tau;  loss_b = dm * dm;  k = -2.0f * dm      (all IEEE)
 *   coef_b = (k * w_b) * grad_scale.    loss[b] = loss_b (NOT weighted);  coef[b] = coef_b: minus d(total loss) / d m, scaled.
 * Gradient, per (r, d): the pair as a group of two in ovla_laplace_pg(_rows)' sum.  g = 0 is the chosen chunk with c_0 = coef_b, or with
 *   c_0 = coef_b + ((nll_coef * w_b) * nll_scale) when nll_coef > 0 (the negative log-likelihood of the chosen chunk beside the preference
 *   loss);  g = 1 is the rejected chunk with c_1 = -coef_b.  A sample with c == 0 is SKIPPED and its chunk is not read.  In ascending g over the
 *   samples not skipped, the first term taken as it is, the second one rounded add, +0 when both are skipped:
 *     acc_mu = sum of (sgn(mu_d - a_{g,d}) * inv_b) * c_g;     acc_s = sum of (1.0f - fabsf(a_{g,d} - mu_d) * inv_b) * c_g
 *   dpred[r, d] = bf16(acc_mu);  dlog_scale[r, d] = inside ? bf16(acc_s) : +0 (inside is true under the by-value scale).  Each optional:
 *   the bits ovla_laplace_pg / ovla_laplace_pg_rows stores at G = 2 for actions (chosen, rejected), advantages (c_0, c_1), grad_scale 1,
 *   no old_logprob and no reference.
 * An observation with w_b == 0 is SKIPPED: none of its chunks, predictions or scales is read, and +0 is stored (set, never multiplied
 *   through) to its rows of logprob, ref_logprob, dpred and dlog_scale and to h, margin, loss and coef: a padding pair full of NaN cannot leak.
 * The stated total is  (1 / B) sum_b w_b loss_b  +  nll_coef (1 / (B chunk)) sum_{b,c} w_b (-lp_w[b, c]);  the caller passes grad_scale =
 * loss_scale / B and nll_scale = loss_scale / (B chunk).
 * Refusals (OVLA_EINVAL, nothing launched): a null pred, ref_pred, chosen, rejected, h, margin, loss or coef; B <= 0; chunk outside
 * [1, OVLA_DPO_CHUNK_MAX]; adim outside [1, 16]; log_scale without ref_log_scale or the reverse; by value: a scale that is not positive and
 * finite; per element: s_lo > s_hi or a bound that is not finite; beta negative, infinite or NaN; nll_coef negative or NaN; label_smoothing
 * outside [0, 0.5) or NaN; loss_type other than 0 or 1; loss_type 1 with beta == 0. */
#define OVLA_DPO_CHUNK_MAX 64
typedef struct {
  const void* pred; const void* ref_pred; const void* log_scale; const void* ref_log_scale;
  const float* chosen; const float* rejected; const float* weight;
  float* logprob; float* ref_logprob; float* h; float* margin; float* loss; float* coef;
  void* dpred; void* dlog_scale;
  float scale[16], log_norm[16];
  float s_lo, s_hi, beta, label_smoothing, grad_scale, nll_coef, nll_scale;
  int32_t loss_type, B, chunk, adim;
} ovla_laplace_dpo_args;
int ovla_laplace_dpo(const ovla_laplace_dpo_args* a, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Value head and generalised advantage estimation (PPO on the L1 head: the Laplace kernels above are the policy's side; these are the
 * critic's).  A value head -- one linear map with adim = 1 on the head's post-layer_norm2 activations -- predicts one number per chunk
 * step; ovla_value_loss pools them into one value per observation and forms the clipped squared-error loss against a return with its
 * gradient; ovla_gae turns a rollout buffer [N trajectories, T steps] into advantages and returns; ovla_advantage_normalize standardises the
 * advantages in place.  All three: stream-ordered, capturable, no atomics, no workspace, nothing read back; every operator written below is
 * one rounded operation of the type named (fp32 unless "double" is said), in the bracketing written, no FMA contraction; a result's bits
 * depend on its own observation / trajectory only, never on where it sits in the batch or on how many others there are (the statistics and
 * the normalisation, which are sums over the batch, in the fixed order written).  THE CONTRACT (identical in csrc/value_gae.hip and in the
 * numpy restatement tests/value_gae_reference.py):
 *
 * ovla_value_loss: u bf16 [B * chunk, 1] (what ovla_head_out_fwd stores for adim = 1; observation b owns rows b * chunk .. + chunk - 1);
 * returns, old_value fp32 [B], valid int32 [B] (each optional); outputs value fp32 [B], du bf16 [B * chunk, 1] (optional; the dpred
 * ovla_head_out_bwd takes), stats fp32 [8].  One workgroup of 64 lanes.  Per observation b:
 *   value    acc = 0;  acc = acc + float(u[b, c]) for ascending c;  v = acc / float(chunk);  value[b] = v, ALWAYS (valid or not).
 *            Without `returns` the launch ends here: du and stats are not touched.
 *   valid    valid[b] != 0, or no `valid`.  Of an observation that is not valid neither returns[b] nor old_value[b] is read, its du rows are
 *            stored as +0 and it enters NO statistic: padding may hold NaN.
 *   error    R = returns[b];  e = v - R;  l = e * e;  dl = e
 *   clipping (value_clip > 0; with value_clip == 0 old_value is not read):  old = old_value[b];  d = v - old;
 *            vc = old + fminf(fmaxf(d, -value_clip), value_clip);  ec = vc - R;  lc = ec * ec;
 *            if lc > l (false on equality and for a NaN): the observation is CLIPPED, l = lc and dl = +0 exactly.
 *   loss     0.5f * l
 *   gradient dl == 0 (clipped, or v == R): the observation's du rows are stored as +0, nothing is multiplied.  Otherwise w = dl * grad_scale
 *            and du[b, c] = bf16_rne(w * inv_chunk) for every c, inv_chunk = 1.0f / float(chunk) formed once on the host.  du is the
 *            gradient with respect to u of  grad_scale * sum_b loss_b.
 *   stats    one lane, over the VALID observations in ascending b, every sum in double (each term converted to double first, each + and
 *            each * one rounded double operation), each rounded to fp32 once at the end:
 *            [0] their number  [1] the number clipped  [2] sum loss  [3] sum v  [4] sum R  [5] sum r * r with r = double(R) - double(v)
 *            [6] sum double(R) * double(R)  [7] +0.   mean loss = [2] / [0], clip fraction = [1] / [0], explained variance =
 *            1 - [5] / ([6] - [4]^2 / [0]).
 * Refusals (OVLA_EINVAL, nothing launched): a null u or value; B <= 0; chunk <= 0; value_clip negative or NaN; with returns: a null stats,
 * a null old_value while value_clip > 0.
 *
 * ovla_gae: reward, value fp32 [N, T], bootstrap fp32 [N] (the value after the last step), done uint8 [N, T] (non-zero: the episode ended
 * AFTER this step), length int32 [N] (optional, default T); gamma and gamma_lambda by value, gamma_lambda = float32(double(gamma) *
 * double(lam)) formed on the host; outputs adv, ret fp32 [N, T].  One lane per trajectory n, len = length[n]:
 *   carry = 0;  for t = len - 1 down to 0:
 *     nd    = done[n, t] ? 0.0f : 1.0f
 *     vnext = (t == len - 1) ? bootstrap[n] : value[n, t + 1]
 *     delta = (reward[n, t] + (gamma * vnext) * nd) - value[n, t]
 *     carry = delta + (gamma_lambda * nd) * carry
 *     adv[n, t] = carry;  ret[n, t] = carry + value[n, t]
 *   Elements t >= len: adv and ret stored as +0, no input of theirs read (with len == 0 not even bootstrap[n]).
 * WHO CHECKS length: the launch reads nothing back, so the HOST side of the call does, on length_host (optional: the same N values in host
 * memory, which the caller that built the buffer holds anyway): an entry outside [0, T] is refused.  The device clamps length[n] to [0, T]
 * before it forms any index, so a bad device value without a host copy cannot leave a buffer; its result is the clamped length's.
 * Refusals: a null reward, value, bootstrap, done, adv or ret; N <= 0; T <= 0; gamma or gamma_lambda outside [0, 1] or NaN; length_host
 * without length; a length_host entry outside [0, T].
 *
 * ovla_advantage_normalize: adv fp32 [N, T] in place, length / length_host as above; the VALID elements are e = n * T + t with t < len_n.
 * One workgroup of 256 lanes; every sum below is taken in this order: lane i adds its valid elements e = i, i + 256, i + 512, ... in
 * ascending e to a double that starts at 0; then the 256 lane sums s[0 .. 255] are folded by s[i] = s[i] + s[i + h] for i < h, h = 128, 64,
 * ..., 1, and the total is s[0].  In double:  count = sum of 1;  mean = (sum of double(x)) / count;  var = (sum of d * d, d = double(x) -
 * mean) / count;  std = sqrt(var) (correctly rounded).  Then in fp32, for every valid element:
 *   adv = (adv - float(mean)) / (float(std) + eps)          (IEEE division)
 * count == 0: nothing is written.  count == 1: mean is the element itself, the result exactly +0.  Elements that are not valid are neither
 * read nor written.  Refusals: a null adv; N <= 0; T <= 0; N * T > 2^20 (one workgroup's reach); eps not positive and finite; length_host
 * as above. */
typedef struct {
  const void* u; const float* returns; const float* old_value; const int32_t* valid;
  float* value; void* du; float* stats;
  float value_clip, grad_scale;
  int32_t B, chunk;
} ovla_value_loss_args;
int ovla_value_loss(const ovla_value_loss_args* a, void* stream);

typedef struct {
  const float* reward; const float* value; const float* bootstrap; const uint8_t* done;
  const int32_t* length; const int32_t* length_host;
  float* adv; float* ret;
  float gamma, gamma_lambda;
  int32_t N, T;
} ovla_gae_args;
int ovla_gae(const ovla_gae_args* a, void* stream);

typedef struct {
  float* adv; const int32_t* length; const int32_t* length_host;
  float eps;
  int32_t N, T;
} ovla_advantage_normalize_args;
int ovla_advantage_normalize(const ovla_advantage_normalize_args* a, void* stream);

/* fp32 -> bf16 convert with scale (publishes .grad views), and fill */
typedef struct { const float* src; void* dst; int64_t n; float scale; } ovla_cvt_args;
int ovla_cvt_f32_to_bf16(const ovla_cvt_args* a, void* stream);
int ovla_cvt_bf16_to_f32(const void* src, float* dst, int64_t n, float scale, void* stream);

/* transpose bf16 [rows, cols] -> [cols, rows] (W^T copies of the frozen weights, LoRA A^T/B^T refresh) */
typedef struct { const void* src; void* dst; int32_t rows, cols; int64_t lds, ldd; } ovla_transpose_args;
int ovla_transpose_bf16(const ovla_transpose_args* a, void* stream);
/* Many transposes in one launch: `table` is a DEVICE array of n ovla_transpose_args (built once: the LoRA factors and
 * their derived A^T / B^T copies never move); `tile_start` is a DEVICE int32 array of n+1 exclusive prefix sums of the
 * entries' 64x64 tile counts, total_tiles = tile_start[n]. */
int ovla_transpose_batched(const ovla_transpose_args* table, const int32_t* tile_start, int32_t n, int32_t total_tiles, void* stream);

/* Grouped, strided 2-D device-to-device copy driven by a device table: one launch moves every tensor of one policy (its LoRA factors into
 * the adapter-slot storage of every adapted linear, its head's and proprio projector's parameter buffers) -- the policy pool's slot swap.
 * Entry i copies `rows` rows of `row_bytes` bytes from src + k src_ld_bytes to dst + k dst_ld_bytes.  Everything is in BYTES and a multiple
 * of 2, pointers are 2-byte aligned; rows == 0 is legal and skipped; with rows > 1 both strides are at least row_bytes.  An entry whose
 * pointers, strides and row_bytes are all multiples of 16 moves 16 bytes per lane (consecutive lanes take consecutive 16-byte pieces of a
 * row, then of the next row: a wave instruction covers whole 64-byte segments of 16 consecutive rows), any other entry 2 bytes per lane;
 * both paths are one kernel.  Exactly the destination rectangles are written; stream-ordered, no atomics, no workspace.  Source and
 * destination rectangles of one table must not overlap each other.
 *
 * ovla_copy_table_plan (host only, no device work): validates n HOST entries and writes the n + 1 exclusive prefix sums of their tile counts
 * to the HOST array tile_start (a tile is at most 16 KiB of one entry: whole rows while a row fits, otherwise 16 KiB pieces of one row).
 * ovla_copy_table: `table` and `tile_start` are the DEVICE copies of what was planned, total_tiles = tile_start[n] (0: nothing to do). */
typedef struct { const void* src; void* dst; int64_t src_ld_bytes, dst_ld_bytes, rows, row_bytes; } ovla_copy_entry;
int ovla_copy_table_plan(const ovla_copy_entry* entries, int32_t n, int32_t* tile_start);
int ovla_copy_table(const ovla_copy_entry* table, const int32_t* tile_start, int32_t n, int32_t total_tiles, void* stream);

/* self-test hook used by tests/: dumps the MFMA / transposed-LDS-read / LDS-DMA lane layouts the kernels rely on.
 * out: fp32 [4, 64, 16] device;  src: bf16 [512] device holding 0..511. */
int ovla_selftest_layouts(float* out, const void* src, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OVLA_H_ */
