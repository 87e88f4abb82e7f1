/*
 * rec_pangu_hip.h — C ABI of librecpangu_hip.so, the MI355X (gfx950) kernels behind the
 * rec_pangu ranking hot path.
 *
 * The reference (HaSai666/rec_pangu v0.4.1) is pure Python over ATen and has NO native
 * interface of its own.  Each entry point below therefore replaces one
 * ATen op *site* of the reference; the site is cited as `file:line` relative to the reference
 * root.  A maintainer binds these with ctypes (rec_pangu_amd/hip.py; INTEGRATION.md shows the
 * stub that goes into the reference's own modules).
 *
 * Conventions
 *   - plain C: raw device pointers + sizes, no torch / C++ types; `stream` is a hipStream_t
 *     passed as void* (0 = the null stream).  All calls are asynchronous on `stream`, never
 *     synchronise, never allocate: every buffer (outputs and workspaces) is owned by the caller.
 *   - pointers named *_ptrs are HOST arrays of DEVICE pointers (copied into the launch packet).
 *   - return 0 on success, <0 on failure (RP_ERR_*); rp_last_error() gives the message for the
 *     calling thread.  Nothing throws or aborts.
 *   - fp32 storage, fp32 accumulation.  Matrix products run on the bf16 matrix core (v_mfma_f32_32x32x16_bf16)
 *     over split-bf16 pieces of the fp32 operands; the number of partial products per flop is the library's
 *     matmul precision (rp_set_matmul_precision, default RP_MATMUL_AUTO: six products = fp32-faithful for
 *     HBM-bound launches, three for matrix-core-bound ones; RP_MATMUL_FP32 = the exact-fp32
 *     v_mfma_f32_32x32x2_f32 reference kernels).
 *   - callable from any host thread (autograd's backward thread included).
 */
#ifndef REC_PANGU_HIP_H
#define REC_PANGU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RP_OK 0
#define RP_ERR_ARG (-1)         /* bad size / alignment / null pointer            */
#define RP_ERR_LAUNCH (-2)      /* hipGetLastError() after a launch                */
#define RP_ERR_UNSUPPORTED (-3) /* shape outside what the kernels were built for   */

#define RP_MAX_FIELDS 64 /* sparse fields (and dense columns) per launch            */

/* epilogue selectors for rp_linear_fwd */
#define RP_ACT_NONE 0
#define RP_ACT_RELU 1
#define RP_ACT_MASK 2 /* out = acc * (aux > 0): ReLU backward fused into a dgrad GEMM */
/* round 5: the other activations rec_pangu/models/layers/activation.py:37-59 hands to an MLP by name, as epilogues of
 * rp_linear_fwd (one extra elementwise launch behind the short-K kernel, fused in the others) */
#define RP_ACT_TANH 3
#define RP_ACT_SIGMOID 4
#define RP_ACT_LEAKY 5 /* nn.LeakyReLU() with its default negative_slope = 0.01 */

/* Matrix-core precision of the GEMM entry points (process-wide; fp32 operands and fp32 accumulation in every mode).
 * The reference computes torch.nn.Linear in fp32 (ATen); BF16X6 reproduces fp32 products to ~2^-23 on the bf16
 * matrix core by splitting each operand into three bf16 pieces (6 MFMA products), BF16X3 to ~2^-16 with two pieces,
 * BF16 rounds the operands to bf16 (outside the 1e-4 parity gate: opt-in only), FP32 uses v_mfma_f32_32x32x2_f32.
 * AUTO (the default) chooses per launch: BF16X3 when the launch is matrix-core bound even at three products
 * (3 x flops / algorithmic bytes above the part's MFMA/HBM ridge of 312), BF16X6 otherwise — HBM-bound launches (every
 * GEMM of the reference's default MLP [64,64,64]) keep the fp32-faithful products at no cost; the model-level parity
 * gates (logits / loss within 1e-4) are tested in AUTO, BF16X6 and forced BF16X3 (tests/test_hip_models.py). */
#define RP_MATMUL_FP32 0
#define RP_MATMUL_BF16 1
#define RP_MATMUL_AUTO 2
#define RP_MATMUL_BF16X3 3
#define RP_MATMUL_BF16X6 6
int rp_set_matmul_precision(int mode); /* default RP_MATMUL_AUTO */
int rp_get_matmul_precision(void);

typedef void *rp_stream_t;

/* ---- library ------------------------------------------------------------------------------ */
#define RP_ABI_VERSION 108 /* rp_version(): bumped with every change of an entry point's prototype (csrc/common.hip) */
int rp_version(void);
const char *rp_last_error(void);
/* number of kernel launches issued through this library since load (tests use it to prove the
 * HIP path, not a fallback, produced a result) */
uint64_t rp_launch_count(void);

/* ---- K1/K2/K3: fused multi-table gather + dense concat + FM second order -------------------
 * replaces  layers/embedding.py:59-63 (F x nn.Embedding + stack),  models/utils.py:122-137
 * (dense stack), ranking/deepfm.py:57-58 (flatten + cat) and layers/interaction.py:38-44 (FM).
 *   arena      [R_total, D] all tables back to back (table f starts at row row_base[f])
 *   row_base   device int64[F];  row_count device int64[F] (= vocab_size+1, bounds check)
 *   idx_ptrs   F device pointers to int64[B] ids (one index per field per sample, bag size 1)
 *   dense_ptrs ND device pointers to float[B]
 *   x          [B, ldx] out: cols [f*D,(f+1)*D) = arena[row_base[f]+idx_f[b]], then ND dense
 *              columns, then zeros up to ldx.  ldx >= F*D+ND.
 *   fm_out     [B]    0.5*sum_d((sum_f v)^2 - sum_f v^2)          (NULL to skip)
 *   sum_out    [B, D] sum_f v, kept for the FM backward           (NULL to skip)
 *   keys_out   int32[F*B], keys_out[f*B+b] = global arena row     (NULL to skip)
 *   err_flag   device int32, set to 1 if any id is outside [0,row_count[f]) (the id is then
 *              clamped to 0; the Python side turns the flag into the reference's IndexError)
 */
int rp_embed_gather_fwd(const float *arena, const int64_t *row_base, const int64_t *row_count,
                        const int64_t *const *idx_ptrs, int F, const float *const *dense_ptrs, int ND,
                        int64_t B, int D, float *x, int64_t ldx, float *fm_out, float *sum_out,
                        int32_t *keys_out, int32_t *err_flag, rp_stream_t stream);

/* The gather FUSED with the Linear (+ ReLU) that consumes its output (DeepFM: embedding.py:59-63 + utils.py:122-137 +
 * deepfm.py:57-58 + interaction.py:38-44 + deep.py:62-72 for dnn.net.0 in ONE launch): the gathered rows go from global
 * memory into MFMA fragments once and are stored to x (NULL: x is not materialised), summed for the FM term and
 * multiplied with the field's 64 x 64 slice of W on the matrix core (split-bf16, six products), so x is never re-read.
 *   W [64, K] (ldw floats per row), K = F*64 + ND;  h1 [B, 64] = relu(x[:, :K] . W^T + bias)
 * rp_embed_gather_linear_fits: D == 64, a 64-wide layer, ND <= 16 (and F <= 32); otherwise RP_ERR_UNSUPPORTED
 * (compose rp_embed_gather_fwd + rp_linear_fwd).
 *   xd [B, 64] (instead of x; NULL otherwise): ONLY the dense columns are stored (zero padded to 64) — the layer's weight
 *   gradient's embedding columns then come from rp_embed_grad_seg and the 4*F*D bytes per sample of the x store (436 MB
 *   at Criteo shape) are never written. */
int rp_embed_gather_linear_fits(int D, int ND, int hidden, int64_t ldx, int64_t ldw);
int rp_embed_gather_linear_fwd(const float *arena, const int64_t *row_base, const int64_t *row_count,
                               const int64_t *const *idx_ptrs, int F, const float *const *dense_ptrs, int ND, int64_t B,
                               int D, float *x, int64_t ldx, const float *W, int64_t ldw, const float *bias, float *h1,
                               float *fm_out, float *sum_out, int32_t *keys_out, int32_t *err_flag, float *xd, rp_stream_t stream);
/* bf16-STORAGE inference (SURVEY D6's secondary mode; the fp32 tables stay the parity path and the training path): the same
 * launch over a bf16 copy of the arena (rows of D bf16 = 128 bytes at D = 64), fp32 accumulation everywhere, nothing stored
 * but h1 and the FM term.  The looked-up values differ from the fp32 tables' by bf16 rounding (2^-9 relative per element):
 * logits within 6e-2 (measured 3.7e-2 at the Criteo shape: tests/test_hip_models.py), not within the 1e-4 parity gate.
 * bf16-STORAGE TRAINING (round 4, secondary mode with a stated tolerance: SURVEY D6): the same launch also stores what the
 * backward needs — x_bf16 [B, ldx] as BF16 (the gathered values are bf16 already: exact; the dense columns are rounded to
 * bf16 for the weight gradient only, the forward uses them in fp32), sum_out [B, 64] fp32, keys_out — all NULL for
 * inference.  The bf16 arena then is the lookup copy the deferred optimizer kernels keep current (rp_lazy_adam_catchup's
 * shadow_bf16); rp_linear_wgrad_xbf16 is the weight gradient over the bf16 activation.  Round 5: with x_bf16 = NULL and
 * xd [B, 64] given (the dense columns in fp32, zero padded — as rp_embed_gather_linear_fwd's xd) NO activation is stored:
 * the weight gradient's embedding columns then come from rp_embed_grad_seg over the fp32 master rows. */
int rp_embed_gather_linear_fwd_bf16(const void *arena_bf16, const int64_t *row_base, const int64_t *row_count,
                                    const int64_t *const *idx_ptrs, int F, const float *const *dense_ptrs, int ND, int64_t B,
                                    int D, const float *W, int64_t ldw, const float *bias, float *h1, float *fm_out,
                                    void *x_bf16, int64_t ldx, float *sum_out, int32_t *keys_out, int32_t *err_flag,
                                    float *xd, rp_stream_t stream);

/* ---- gather backward: sort by arena row, then segmented reduce into the dense grad arena ----
 * replaces aten::embedding_dense_backward under layers/embedding.py:62 and the autograd of
 * interaction.py:38-44.  rp_sort_pairs_i32 sorts (key, position) pairs by the low end_bit bits of the key
 * (stable, so equal rows keep ascending sample order; end_bit = 32 orders the keys as SIGNED ints);
 * position = index into keys_in.  keys_in / keys_out / pos_out must not alias.  Kernel launches only (no
 * memset, nothing carried between calls): capturable into a hipGraph at any n.  Workspace size from
 * rp_sort_workspace_bytes. */
int rp_sort_workspace_bytes(int64_t n, size_t *bytes);
int rp_sort_pairs_i32(void *workspace, size_t workspace_bytes, const int32_t *keys_in, int32_t *keys_out,
                      int32_t *pos_out, int64_t n, int end_bit, rp_stream_t stream);
/* The same sort for the pair list of ONE lookup over F tables that sit in the arena in field order (round 6; csrc/sort.hip):
 * keys_in[f * B + b] = arena row of pair (field f, sample b) (rp_embed_keys); field_base / field_rows: host arrays [F], first
 * arena row and row count of each field's table.  The list is sorted segment by segment — a field's B pairs by the row inside
 * its table, ceil(log2 rows) key bits instead of the arena's — and comes out as rp_sort_pairs_i32(end_bit = bits of the arena)
 * gives it, bit for bit (the stable sort by arena row; pos_out = field * B + sample).  9-bit passes over the fields that still
 * have bits left: 49 field-passes instead of 78 at Criteo shape.  Kernel launches only; workspace from
 * rp_sort_pairs_fields_workspace_bytes(B, F). */
int rp_sort_pairs_fields_workspace_bytes(int64_t B, int F, size_t *bytes);
int rp_sort_pairs_fields_i32(void *workspace, size_t workspace_bytes, const int32_t *keys_in, int32_t *keys_out,
                             int32_t *pos_out, int64_t B, int F, const int64_t *field_base, const int64_t *field_rows,
                             rp_stream_t stream);
/*   grad_arena[key] (+)= sum over pairs p=(f,b) with that key of
 *        dx[b, f*D:(f+1)*D]  +  (gfm ? gfm[b] * (sum_in[b,:] - arena[key,:]) : 0)
 *        (sum_in may be NULL with gfm given: the gfm[b]*sum_in[b,:] part was already added to dx by
 *         rp_linear_fwd_rowadd, only the -gfm[b]*arena[key,:] part is applied here)
 *   dx may be NULL (FM-only models), gfm may be NULL (no FM term), not both.
 *   accumulate=0: every row that has pairs is OVERWRITTEN with its sum (rows without pairs are not touched: the caller
 *                 keeps them zero, rp_zero_rows);   accumulate=1: the sum is added to what is there.
 *   Deterministic: every row has one writer and every sum a fixed order (ascending sorted position — the sort is
 *   stable, so ascending sample index); runs that cross workgroups are chained through `workspace`
 *   (rp_embed_grad_reduce_workspace_bytes) by a second launch.  No floating-point atomics.                        */
int rp_embed_grad_reduce_workspace_bytes(int64_t n, int D, size_t *bytes);
int rp_embed_grad_reduce(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int64_t B, int D,
                         const float *dx, int64_t ldx, const float *gfm, const float *sum_in,
                         const float *arena, float *grad_arena, int accumulate, void *workspace,
                         size_t workspace_bytes, rp_stream_t stream);
/* The same reduce FUSED with the dgrad of the Linear that consumes the gathered rows (DeepFM's dnn.net.0, deep.py:62-72 +
 * embedding.py:62): the dX row of pair (f, b) is dh[b, 0:64] . W1[:, f*64:(f+1)*64], formed on the matrix core
 * (split-bf16, six products) inside the reduce, so the [B, F*D] gradient of the MLP input is never written or read.
 *   dh  [B, 64]            gradient w.r.t. the layer's pre-activation (lddh floats per row)
 *   wt  [>= F*64, 64]      the layer's weight transposed (rp_transpose): row f*64+d = column f*64+d of W1 [64, K]
 *   dx  optional           sum of the gradients of x's other consumers, added per pair (NULL: none)
 *   skip_fields            bit f set: the pairs of field f are left out (their tables' gradient rows come from
 *                          rp_embed_grad_tiny); only with FIELD-MAJOR positions (position = field * B + sample), 0 otherwise
 * rp_embed_grad_gemm_fits: D == 64, a 64-wide layer, row strides multiples of 4 floats; otherwise RP_ERR_UNSUPPORTED
 * (compose rp_linear_fwd + rp_embed_grad_reduce).  Workspace: rp_embed_grad_reduce_workspace_bytes(n, D). */
int rp_embed_grad_gemm_fits(int D, int hidden, int64_t lddh, int64_t ldwt);
int rp_embed_grad_gemm(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int64_t B, int D, const float *dh,
                       int64_t lddh, const float *wt, int64_t ldwt, const float *dx, int64_t ldx, const float *gfm,
                       const float *sum_in, const float *arena, float *grad_arena, int accumulate, uint64_t skip_fields,
                       void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* The same gradient for TINY tables (each <= 254 rows, <= 224 rows together, <= 16 tables), SAMPLE-major (csrc/embed_tiny.hip):
 * G[r] = (sum_b dH[b]) . W1_f^T + sum_b g_fm[b] S[b] - (sum_b g_fm[b]) v_r over the samples b with id_f[b] = r; the 129-wide row
 * sums are one-hot GEMMs on the matrix core (one-hot exact in bf16, the data split into three bf16 pieces, fp32 accumulation
 * in a fixed order: deterministic), every sample's dH / S row is read once for all tiny tables.  Writes the rows somebody
 * looked up in this batch (accumulate != 0 adds), like rp_embed_grad_gemm: other rows are not touched.  keys [F * B]: arena row of pair (field, sample) at
 * field * B + sample (rp_embed_keys / the gather's keys_out).  Host arrays: tiny_field (field index), tiny_base (first arena
 * row), tiny_rows.  rp_embed_grad_gemm(skip_fields = bits of those fields) then covers the other fields.  dw != NULL
 * (round 5): also  dw[:, f*64:(f+1)*64] = sum over the table's rows of  (sum_b dH[b])^T (x) v_r  — the tiny tables' columns
 * of the first layer's weight gradient (see rp_embed_grad_seg); a table row nobody looked up in this batch contributes
 * nothing, whatever it holds (like the sorted forms, which never read it).  Needs arena and lddw >= (field + 1) * 64 for
 * every table.  Every argument is checked in front of the first launch: a refused call has written nothing. */
int rp_embed_grad_tiny_workspace_bytes(int64_t B, size_t *bytes);
int rp_embed_grad_tiny(const int32_t *keys, int64_t B, const int32_t *tiny_field, const int64_t *tiny_base,
                       const int32_t *tiny_rows, int n_tiny, const float *dh, int64_t lddh, const float *wt, int64_t ldwt,
                       const float *gfm, const float *sum_in, const float *arena, float *grad_arena, int accumulate,
                       float *dw, int64_t lddw, void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* The first layer's WHOLE backward on the embedding columns, segment-sum first (csrc/embed.hip, round 5; replaces
 * rp_embed_grad_gemm + the rp_linear_wgrad over a stored activation on the single-device path).  Reference ops:
 * aten::embedding_dense_backward of rec_pangu/models/layers/embedding.py:61-63, the `** 2` backward of
 * layers/interaction.py:38-44, the first Linear's dgrad and the embedding columns of its weight gradient
 * (layers/deep.py:62-72 on the input built at ranking/deepfm.py:57-59).  Per run of equal keys in the row-sorted pair list
 * (pairs p = (f, b) of one table row r):  Hs = sum dh[b, :],  u = sum gfm[b] sum_in[b, :],  s = sum gfm[b];
 *     grad_arena[r, :] (+)= Hs . w[:, f*64:(f+1)*64] + u - s arena[r, :]
 *     dw[:, f*64:(f+1)*64]  = sum over the field's runs of  Hs^T (x) arena[r, :]      (dw != NULL; written, not added)
 * w = the layer's weight [64, ldw] (row-major, NOT transposed), dh [B, 64] the gradient of its pre-activation.  FIELD-MAJOR
 * positions only: sorted_pos[i] = field * B + sample, n = F * B, F <= 64.  skip_fields: bit f set = field f is left out
 * (its table is rp_embed_grad_tiny's, which fills the same dw columns when given dw).  field_rows: host array [F] of table
 * sizes (scheduling only: long chunks first) or NULL.  gfm and sum_in both NULL = no FM term.  Deterministic (one writer
 * per row, fixed summation orders).  Workspace: rp_embed_grad_seg_workspace_bytes(n, B, D).
 * rp_embed_grad_seg_fits: D == 64, a 64-wide layer, lddh % 4 == 0; otherwise RP_ERR_UNSUPPORTED. */
int rp_embed_grad_seg_fits(int D, int hidden, int64_t lddh);
int rp_embed_grad_seg_workspace_bytes(int64_t n, int64_t B, int D, size_t *bytes);
int rp_embed_grad_seg(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int64_t B, int D, const float *dh,
                      int64_t lddh, const float *w, int64_t ldw, const float *gfm, const float *sum_in, const float *arena,
                      float *grad_arena, int accumulate, uint64_t skip_fields, const int64_t *field_rows, float *dw,
                      int64_t lddw, void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* rp_embed_grad_seg's work in two launches (csrc/embed_ss.hip, round 6; the same reference ops, contract and results up to
 * fp32 summation order): a STREAMING segment-sum pass with no LDS and no barrier (a 16-lane group per 32 sorted positions
 * writes one record [sum dh | sum gfm sum_in | sum gfm] per run piece) and a matrix pass over tiles of 128 UNIQUE rows of a
 * field (a row's pieces summed in position order first; one writer per row, no run is cut at a tile border).  This form is
 * for the tables whose runs are long (the mid-size ones: rp_embed_grad_smp takes the big tables, rp_embed_grad_tiny the
 * tiny ones).
 * The matrix pass reads the fields' unique-row lists (ustart, ukey, offs): rp_embed_grad_ss_mark makes them from the sorted
 * keys alone (three short launches — with the sort, a step ahead); NULL x 3 = made inside this call (workspace).  Sizes in
 * int32 elements: rp_embed_grad_ss_mark_sizes(B, kept fields) -> n_rows (ustart and ukey each), n_offs.
 * phases: 1 = the segment-sum launch (reads dh / sum_in / gfm and the sorted pairs only), 2 = the launches behind it (same
 * workspace, ordered behind phase 1), 3 = both.  Workspace: rp_embed_grad_ss_workspace_bytes(n, B, D, skip_fields). */
int rp_embed_grad_ss_workspace_bytes(int64_t n, int64_t B, int D, uint64_t skip_fields, size_t *bytes);
int rp_embed_grad_ss_mark_sizes(int64_t B, int n_kept, size_t *n_rows, size_t *n_offs);
int rp_embed_grad_ss_mark(const int32_t *sorted_keys, int64_t n, int64_t B, uint64_t skip_fields, int32_t *ustart, int32_t *ukey,
                          int32_t *offs, rp_stream_t stream);
int rp_embed_grad_ss(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int64_t B, int D, const float *dh,
                     int64_t lddh, const float *w, int64_t ldw, const float *gfm, const float *sum_in, const float *arena,
                     float *grad_arena, int accumulate, uint64_t skip_fields, const int64_t *field_rows, float *dw,
                     int64_t lddw, const int32_t *ustart, const int32_t *ukey, const int32_t *offs, int phases,
                     void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* The same backward for the BIG tables, SAMPLE-major (csrc/embed_smp.hip, round 6; reference ops as rp_embed_grad_seg:
 * rec_pangu/models/layers/embedding.py:61-63 backward, layers/interaction.py:38-44 backward, layers/deep.py:62-72 dgrad and
 * the embedding columns of the weight gradient).  For a table whose runs in the sorted pair list are mostly singletons the
 * sort buys nothing and the (field, row) order re-gathers every sample's dh / sum_in row once per field; this launch walks
 * the batch in sample order instead (a unit = 64 samples x one field: dh staged once in LDS, the table rows gathered into
 * the matrix core's accumulator layout, dgrad + FM term + the field's weight-gradient columns from the same registers):
 *     pair (f, b), r = keys[f * B + b]:   row = dh[b, :] . w[:, f*64:(f+1)*64] + gfm[b] (sum_in[b, :] - arena[r, :])
 *     grad_arena[r, :] (+)= row                       when the pair is alone in its run of the sorted list (one writer), else
 *     the row goes to a side buffer at its number among such pairs and rp_embed_grad_reduce_rows sums the runs in list order;
 *     dw[:, f*64:(f+1)*64] = sum_b dh[b, :]^T (x) arena[r, :]                      (dw != NULL; written, not added)
 * rp_embed_grad_smp_mark (from the sorted list; may run ahead of the backward: it depends on the batch's ids only): the
 *     pairs whose run has >= 2 pairs are numbered c = 0, 1, ... in sorted order (field by field);
 *     dupq[fi * B + b] = c of pair (fields[fi], b), or -1 for a pair alone in its run;  dupkeys[c] = the key of pair c, -1
 *     from the number of such pairs on.  Both [n_fields * B] int32, caller-owned; scratch: rp_embed_grad_smp_mark_scratch
 *     int32 words.
 * fields: host array, ascending, <= 16; field_base / field_rows: host arrays [n_fields], first arena row and row count of each
 * field's table (< 2^24 rows: 32-bit row offsets; n_fields * B < 2^24); FIELD-MAJOR positions (n = F * B, F <= 64).
 * rp_embed_grad_seg(skip_fields = their bits) covers the other fields.  phases: 1 = the main launch, 2 = the launches behind it
 * (the partial sums of dw, the duplicate runs: they touch no row of another launch and may run beside rp_embed_grad_seg on a
 * second stream, ordered behind phase 1 on the same workspace), 3 = both.  Deterministic.  Workspace: rp_embed_grad_smp_workspace_bytes(B, n_fields).
 * rp_embed_grad_reduce_rows: grad_arena[key, :] (+)= sum of rows[i, :] over the entries i of a key-sorted list with
 * keys[i] == key; key -1 = no entry (its row is not read).  Workspace: rp_embed_grad_reduce_workspace_bytes(n, D). */
int rp_embed_grad_smp_fits(int D, int hidden, int64_t lddh);
int rp_embed_grad_smp_workspace_bytes(int64_t B, int n_fields, size_t *bytes);
int rp_embed_grad_smp_mark_scratch(int64_t B, int n_fields, size_t *n_int32);
int rp_embed_grad_smp_mark(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int64_t B,
                           const int32_t *fields, int n_fields, int32_t *dupq, int32_t *dupkeys, int32_t *scratch,
                           rp_stream_t stream);
int rp_embed_grad_smp(const int32_t *keys, const int32_t *dupq, const int32_t *dupkeys, int64_t B, int F,
                      const int32_t *fields, const int64_t *field_base, const int64_t *field_rows, int n_fields,
                      const float *dh, int64_t lddh, const float *w, int64_t ldw,
                      const float *gfm, const float *sum_in, const float *arena, float *grad_arena, int accumulate,
                      float *dw, int64_t lddw, int phases, void *workspace, size_t workspace_bytes, rp_stream_t stream);
int rp_embed_grad_reduce_rows(const int32_t *keys, const float *rows, int64_t n, int D, float *grad_arena, int accumulate,
                              void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* grad_arena[keys[i], :] = 0 for i < n (duplicates allowed) */
int rp_zero_rows(const int32_t *keys, int64_t n, int D, float *grad_arena, rp_stream_t stream);
/* dst[0 .. n_words) = value, 32-bit words, 16-byte aligned buffer: the library's own fill (a recorded step must hold no
 * ATen fill kernel / memset node: csrc/plan.hip) */
int rp_fill_words(void *dst, int64_t n_words, uint32_t value, rp_stream_t stream);

/* ---- K4: Linear (+bias +activation) on the fp32 MFMA ----------------------------------------
 * replaces layers/deep.py:62-72 (nn.Linear + ReLU chain) and its autograd.
 *   out[M,N] = act(a[M,K] . w[N,K]^T + bias[N]);  bias may be NULL;
 *   act = RP_ACT_MASK multiplies by (aux[m,n] > 0) (aux: [M, ldaux]); RP_ACT_TANH / SIGMOID / LEAKY: see above. */
int rp_linear_fwd(const float *a, int64_t lda, const float *w, int64_t ldw, const float *bias, float *out,
                  int64_t ldo, int64_t M, int N, int K, int act, const float *aux, int64_t ldaux,
                  rp_stream_t stream);
/* weight/bias gradient: dw[N,K] (+)= dy[M,N]^T . x[M,K];  db[N] (+)= column sums of dy.
 * Deterministic two-stage reduction through `workspace` (rp_linear_wgrad_workspace_bytes).  */
int rp_linear_wgrad_workspace_bytes(int64_t M, int N, int K, size_t *bytes);
int rp_linear_wgrad(const float *dy, int64_t lddy, const float *x, int64_t ldx, float *dw, int64_t lddw,
                    float *db, int64_t M, int N, int K, int accumulate, void *workspace,
                    size_t workspace_bytes, rp_stream_t stream);
/* the same with the activation stored as bf16 (x_bf16 [M, ldx] bf16, ldx even, 4-byte aligned; the bf16-storage training
 * mode): half the bytes of the dominant operand; bf16 matrix-core modes and N < 128 only (RP_ERR_UNSUPPORTED otherwise) */
int rp_linear_wgrad_xbf16(const float *dy, int64_t lddy, const void *x_bf16, int64_t ldx, float *dw, int64_t lddw,
                          float *db, int64_t M, int N, int K, int accumulate, void *workspace, size_t workspace_bytes,
                          rp_stream_t stream);
/* Which launch form the three entry points above choose for a shape, under the matmul precision in force.  Pure host
 * functions (no device call): the entry points switch on the same result.  `out` receives RP_GEMM_FORM_INTS ints, indexed
 * by the slots below; slots a family does not use are 0.
 *   rp_linear_fwd_form:   a_aligned16 / w_aligned16 = the pointer is 16-byte aligned.  RP_GEMM_FWD_COLSPLIT issues
 *     rp_linear_fwd on [M, SPLIT_NB] and on [M, N - SPLIT_NB] (same strides and alignment), each with a form of its own.
 *   rp_linear_wgrad_form: x_align_bytes = the largest power of two (<= 16) dividing the address of x; x_is_bf16 = 1 asks
 *     for rp_linear_wgrad_xbf16 and returns RP_ERR_UNSUPPORTED exactly where that entry point does. */
#define RP_GEMM_FORM_INTS 16
#define RP_GEMM_FAMILY 0 /* RP_GEMM_FWD_* / RP_GEMM_WGRAD_* */
#define RP_GEMM_NPROD 1  /* matrix-core products per flop: 0 (an f32 kernel), 1, 3, 6 */
#define RP_GEMM_FWD_TILE 2        /* tiled: RP_GEMM_TILE_* */
#define RP_GEMM_FWD_VEC_A 3       /* rows of a fetched as 16-byte vectors (lda % 4 == 0, aligned pointer) */
#define RP_GEMM_FWD_VEC_W 4
#define RP_GEMM_FWD_SK_LAUNCHES 5 /* short K: RP_GEMM_SK_* bits, the launches issued */
#define RP_GEMM_FWD_SK_PER 6      /* short K: column tiles per workgroup of the first launch */
#define RP_GEMM_FWD_GRID_X 7      /* grid of the (first) launch */
#define RP_GEMM_FWD_GRID_Y 8
#define RP_GEMM_FWD_POST_ACT 9    /* an rp_act_fwd launch follows in place (tanh / sigmoid / leaky behind short K) */
#define RP_GEMM_FWD_SPLIT_NB 10   /* column split: the columns of the first launch */
#define RP_GEMM_WGRAD_NA 2        /* 64-column output tiles per workgroup (bf16 kernels) */
#define RP_GEMM_WGRAD_VEC_X 3     /* f32 kernel: 16-byte rows of x; bf16 kernels: 8-byte rows (1 for a bf16 activation) */
#define RP_GEMM_WGRAD_VEC_Y 4     /* f32 kernel only */
#define RP_GEMM_WGRAD_S 5         /* batch splits = partial results in the workspace */
#define RP_GEMM_WGRAD_ROWS 6      /* batch rows per split */
#define RP_GEMM_WGRAD_GRID_X 7
#define RP_GEMM_WGRAD_GRID_Y 8
#define RP_GEMM_WGRAD_GRID_Z 9
#define RP_GEMM_FWD_F32 0
#define RP_GEMM_FWD_SHORTK 1
#define RP_GEMM_FWD_COLSPLIT 2
#define RP_GEMM_FWD_WIDE 3  /* 256 x 128 tiles */
#define RP_GEMM_FWD_TILED 4
#define RP_GEMM_TILE_128X128 0   /* eight waves */
#define RP_GEMM_TILE_128X64_8W 1 /* eight waves */
#define RP_GEMM_TILE_128X64_4W 2 /* four waves */
#define RP_GEMM_SK_INTERIOR 1 /* the straight-line kernel over the whole 128 x 64 tiles */
#define RP_GEMM_SK_RIGHT 2    /* guarded: all rows, the last partial column tile */
#define RP_GEMM_SK_BOTTOM 4   /* guarded: the last rows over the interior columns */
#define RP_GEMM_SK_GUARDED 8  /* no interior: one guarded launch over everything */
#define RP_GEMM_WGRAD_F32 0
#define RP_GEMM_WGRAD_NARROW 1 /* 64 x 128 output tiles */
#define RP_GEMM_WGRAD_WIDE 2   /* 128 x 128 output tiles, XCD-local 1-D grid */
#define RP_GEMM_WGRAD_XBF16 3
int rp_linear_fwd_form(int64_t M, int N, int K, int64_t lda, int64_t ldw, int a_aligned16, int w_aligned16, int act,
                       int *out);
int rp_linear_wgrad_form(int64_t M, int N, int K, int64_t lddy, int64_t ldx, int dy_aligned16, int x_align_bytes,
                         int x_is_bf16, int *out);
/* out[C,R] = in[R,C]^T (weights for the dgrad GEMM); rows C .. C_out-1 of out (C_out >= C) are written as zeros */
int rp_transpose(const float *in, int64_t ldin, float *out, int64_t ldout, int R, int C, int C_out, rp_stream_t stream);
/* rp_transpose and rp_copy_rows of the same matrix in ONE launch: out = in^T as rp_transpose, copy[r, 0:C] = in[r, 0:C] with
 * row stride ldcopy (the first layer's weight: its transposed copy for the gather backward and its aligned copy for the
 * gather forward are both made in front of the forward) */
int rp_transpose_copy(const float *in, int64_t ldin, float *out, int64_t ldout, int R, int C, int C_out, float *copy,
                      int64_t ldcopy, rp_stream_t stream);
/* out[r, 0:C] = in[r, 0:C], r < R, with another row stride (staging copy of a weight with unaligned rows) */
int rp_copy_rows(const float *in, int64_t ldin, float *out, int64_t ldout, int R, int C, rp_stream_t stream);
/* out[r, 0:C] += in[r, 0:C] (independent row strides): the gradient of a column block of the gathered activation that a
 * second consumer produced (AutoInt's attention over x[:, :F*D], autoint.py:44-46) added into the first consumer's dX */
int rp_add_rows(const float *in, int64_t ldin, float *out, int64_t ldout, int R, int C, rp_stream_t stream);
/* ---- nn.Linear forward on PRE-SPLIT bf16 operands (csrc/gemm_pieces.hip; round 4) ---------------------------------
 * Same contract as rp_linear_fwd (deep.py:62-72: out = act(a . w^T + bias)), but both operands arrive as bf16 PIECES in
 * the "interleaved" layout: a row is a sequence of 128-byte k-tiles,
 *   np = 2 (the bf16x3 products hi.lo + lo.hi + hi.hi):  [32 x bf16 hi | 32 x bf16 lo]  per 32 values of K
 *   np = 1 (plain bf16, a stated-tolerance mode):        [64 x bf16]                    per 64 values of K
 * K zero-padded to whole tiles: a row holds rp_pieces_ld(K, np) bf16 elements (lda / ldw >= that, multiples of 8).  The
 * k-tiles go HBM -> LDS by LDS-DMA and the inner loop is fragment reads and MFMAs only.  np = 2 is bit-identical to
 * rp_linear_fwd under RP_MATMUL_BF16X3.  rp_pieces_pack makes the layout from an fp32 matrix [M, K] (hi = RN(x),
 * lo = RN(x - hi)); ldo in bf16 elements, a multiple of 64.  act: RP_ACT_NONE / RELU / MASK (aux as in rp_linear_fwd). */
int64_t rp_pieces_ld(int K, int np);
int rp_pieces_pack(const float *in, int64_t ld, int64_t M, int K, int np, void *out, int64_t ldo, rp_stream_t stream);
int rp_linear_fwd_pieces(const void *a, int64_t lda, const void *w, int64_t ldw, const float *bias, float *out,
                         int64_t ldo, int64_t M, int N, int K, int np, int act, const float *aux, int64_t ldaux,
                         rp_stream_t stream);
/* y = dy * (act_out > 0), elementwise over [M,N] */
int rp_relu_bwd(const float *dy, int64_t lddy, const float *act_out, int64_t ldact, float *out, int64_t ldo,
                int64_t M, int N, rp_stream_t stream);
/* the activations as launches of their own (elementwise over [M,N]; act = RP_ACT_RELU / TANH / SIGMOID / LEAKY):
 * rp_act_fwd: y = act(x) (y == x allowed);  rp_act_bwd: out = dy * act'(.) expressed through the activation's OUTPUT
 * (relu / leaky: sign of y; tanh: 1 - y^2; sigmoid: y (1 - y)) — the backward of rp_linear_fwd(act) needs no pre-activation */
int rp_act_fwd(const float *x, int64_t ldx, float *y, int64_t ldy, int64_t M, int N, int act, rp_stream_t stream);
int rp_act_bwd(const float *dy, int64_t lddy, const float *act_out, int64_t ldact, float *out, int64_t ldo, int64_t M,
               int N, int act, rp_stream_t stream);

/* ---- K5: DCN-v1 CrossNet, all L layers in one pass ------------------------------------------
 * replaces layers/interaction.py:119-141 (CrossInteractionLayer/CrossNet) and, when wfc is given,
 * the `fc` that follows it in ranking/dcn.py:64.
 *   X_{l+1} = X_l + (X_l . W[l]) * X_0 + Bv[l];   W, Bv: [L, d] (the L Linear(d,1) weights / biases stacked)
 *   xout [B, ldo] = X_L (NULL to skip);  logit[B] = X_L . wfc + bfc[0] (NULL to skip)
 *   s_out [B, L] = the per-layer scalars X_l . W[l], all the backward needs besides X_0.
 * backward: rp_crossnet_bwd_rows below.  d <= 2048, L <= 6.        */
int rp_crossnet_fwd(const float *x0, int64_t ldx, int d, int L, const float *W, const float *Bv, const float *wfc,
                    const float *bfc, float *xout, int64_t ldo, float *logit, float *s_out, int64_t B,
                    rp_stream_t stream);

/* ---- K6: xDeepFM CIN layer on the fp32 MFMA ------------------------------------------------------
 * replaces layers/interaction.py:164-168 (einsum "bhd,bmd->bhmd" + view + Conv1d(k=1) + sum over d).
 *   x0 [B, ld0]: X_0[b] as H rows of D floats;  xp [B, ldp]: X_{k-1}[b] as M rows of D floats (xp == x0 for layer 1)
 *   W  [O, H*M] (Conv1d weight, channel c = h*M + m), bias [O] or NULL
 *   out [B, O, D] = X_k (NULL to skip: the collapsed last layer only needs the pooling)
 *   pooled [B, ldpool]: pooled[b, o] = sum_d X_k[b,o,d]  (NULL to skip)
 * The outer product [B, H*M, D] is never materialised.  H <= 32 fields; must fit the 160 KB LDS.
 * backward (g_out [B,O,D] = dL/dX_k and/or g_pool [B, ldgp] = dL/dpooled, broadcast over d):
 *   rp_cin_layer_bwd_x: dx0 [B, lddx0] (+)= , dxp [B, lddxp] = gradients of both factors
 *   rp_cin_layer_bwd_w: dW [O, H*M], dbias [O] (batch-reduced through `workspace`)                           */
int rp_cin_layer_fwd(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *W, const float *bias,
                     float *out, float *pooled, int64_t ldpool, int H, int M, int O, int D, int64_t B,
                     rp_stream_t stream);
/* add_dx0 != 0: dx0 += (several layers share X_0), else dx0 = ; for the first layer (xp == x0) both factor
 * gradients land in dx0 and dxp is ignored.  Middle layers with O >= 4 need M <= 32 (register-tiled). */
int rp_cin_layer_bwd_x(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *W, const float *g_out,
                       const float *g_pool, int64_t ldgp, float *dx0, int64_t lddx0, int add_dx0, float *dxp,
                       int64_t lddxp, int H, int M, int O, int D, int64_t B, rp_stream_t stream);
int rp_cin_layer_bwd_w_workspace_bytes(int64_t B, int H, int M, int O, size_t *bytes);
int rp_cin_layer_bwd_w(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *g_out,
                       const float *g_pool, int64_t ldgp, float *dW, float *dbias, int H, int M, int O, int D,
                       int64_t B, void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- K7: AutoInt field self-attention layer ----------------------------------------------------
 * replaces layers/attention.py:63-101 (MultiHeadSelfAttention, align_to="output", no dropout/LayerNorm):
 * QKV(+residual) projections, RAW-view head split (:73-75), scores [/scale], softmax, PV, +residual, ReLU.
 *   x   [B, ldx]: T tokens of Din floats, contiguous per sample (x[b, t*Din + k])
 *   W   [(3|4)*H*a, Din]: Wq, Wk, Wv (and Wres when has_res) stacked; without Wres Din must equal H*a
 *   scale: attention_dim**0.5 when use_scale, 0 for none
 *   out [B, T*H*a];   backward: gout [B, T*H*a] -> dx [B, lddx] (NULL to skip), dW like W.          */
int rp_field_attention_fits(int T, int Din, int H, int a, int has_res); /* 1 if fwd+bwd fit the 160 KB LDS */
int rp_field_attention_fwd(const float *x, int64_t ldx, const float *W, int T, int Din, int H, int a, int has_res,
                           float scale, float *out, int64_t B, rp_stream_t stream);
int rp_field_attention_bwd_workspace_bytes(int64_t B, int T, int Din, int H, int a, int has_res, size_t *bytes);
int rp_field_attention_bwd(const float *x, int64_t ldx, const float *W, int T, int Din, int H, int a, int has_res,
                           float scale, const float *gout, float *dx, int64_t lddx, float *dW, int64_t B,
                           void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- K8: MMOE gate softmax + gate-weighted expert combine -----------------------------------
 * replaces multi_task/mmoe.py:92-104.  The expert einsum (mmoe.py:86) and the T gate products (:94)
 * are ONE rp_linear_fwd over the concatenated [experts | gates] matrix; its output z [B, ldz] has the
 * expert outputs at columns k*E+e (k < K) and the gate logits at K*E + t*E + e.
 *   gate [B, T*E] = per-task softmax over experts (kept for the backward)
 *   out  [T, B, K] : out[t,b,k] = sum_e z[b,k*E+e] * gate[b,t,e]
 * backward: dout [T,B,K] -> dz [B, lddz] (expert columns and gate-logit columns).  T, E <= 8, T*E <= 32. */
int rp_mmoe_combine_fwd(const float *z, int64_t ldz, int K, int E, int T, float *out, float *gate, int64_t B,
                        rp_stream_t stream);
int rp_mmoe_combine_bwd(const float *z, int64_t ldz, int K, int E, int T, const float *gate, const float *dout,
                        float *dz, int64_t lddz, int64_t B, rp_stream_t stream);

/* Streaming CrossNet backward.  X_l = A_l X_0 + C_l (A_l = 1 + sum_{k<l} s_k per sample,
 * C_l = sum_{k<l} b_k per feature), so one wave per row produces dx0 and V[B, 2L+2] =
 * [t_l A_l (l<L) | g_logit A_L | t_l (l<L) | g_logit]; then dW_l = (V^T X_0)[l] + C_l colsum(V)[L+1+l] etc. are one
 * rp_linear_wgrad(V, X_0) plus [L,d]-sized weight-space arithmetic.  d <= 2048.                            */
int rp_crossnet_bwd_rows(const float *x0, int64_t ldx, int d, int L, const float *W, const float *wfc,
                         const float *s_in, const float *g_x, int64_t ldg, const float *g_logit, float *dx0,
                         int64_t lddx, float *V, int64_t B, rp_stream_t stream);
/* the CrossNet's parameter gradients from P [2L+2, ldp] = V^T X_0 (rp_linear_wgrad over V) and cs [2L+2] = column sums of V:
 * dW [L, d], dB [L, d] and — with the fused fc (wfc [d]) — dwfc [d]; colg [d] = column sums of the incoming gradient when
 * there is no fused fc (else NULL).  One launch for what autograd of interaction.py:119-141 spreads over the layers. */
int rp_crossnet_param_grads(const float *P, int64_t ldp, const float *cs, const float *W, const float *Bv, const float *wfc,
                            const float *colg, int L, int d, float *dW, float *dB, float *dwfc, rp_stream_t stream);

/* ---- K6 (bf16 matrix core): a CIN layer with at most 32 x 32 (field, map) pairs per channel ----------------
 * replaces interaction.py:157-171 for such a layer (a FIRST layer: X_{k-1} = X_0, H = M <= 32) on
 * v_mfma_f32_32x32x16_bf16 with split-bf16 operands (fp32-faithful, 6 products).  The X_{k-1} fragments stay in
 * registers, the channels' weights stream past as bf16 pieces  wp [O][3][32][32]  = (hi, mid, lo) of W[o, row, col]
 * zero-padded to 32 x 32 (hi = bf16(w), mid = bf16(w - hi), lo = bf16(w - hi - mid)).
 *   fwd   : out [B, O, D] and/or pooled [B, O] (= sum_d out); bias [O] optional
 *   bwd_x : dx[b,r,:] = sum_o (gout[b,o,:] + gpool[b,o]) sum_c wp[o][r][c] xk[b,c,:]   — X_0-role gradient with
 *           wp from W[o,h,m], X_{k-1}-role gradient with W[o,m,h]; for a first layer W[o,h,m] + W[o,m,h] gives the
 *           whole gradient in one pass.
 * Limits: rows, contraction <= 32, D in {32, 64} (rp_cin_bs_fits). */
int rp_cin_bs_fits(int H, int M, int D);
/* A layer fed by MORE than 32 maps (a middle layer of e.g. cin_layer_units = [128, 128, 128]) is the sum over chunks of
 * <= 32 maps of such layers: rp_cin_bs_fwd per chunk (xp = the chunk's columns of X_{k-1}, leading dimension M*D),
 * partial outputs summed with rp_accumulate; in the backward g_out is shared, rp_cin_bs_bwd_x gives the X_0-role
 * gradient per chunk (accumulated) and the chunk's own X_{k-1}-role gradient (written into its columns), and
 * rp_cin_bs_bwd_w the chunk's slice of dW (functional._CINChunked).  dst[0:n] += src[0:n]: */
int rp_accumulate(float *dst, const float *src, int64_t n, rp_stream_t stream);
int rp_cin_bs_fwd(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const void *wp, const float *bias, int H,
                  int M, int O, int D, float *out, float *pooled, int64_t B, rp_stream_t stream);
int rp_cin_bs_bwd_x(const float *xk, int64_t ldk, const void *wp, const float *gout, const float *gpool, int R, int Cn,
                    int O, int D, float *dx, int64_t lddx, int64_t B, rp_stream_t stream);
/* dW [O, H*M], db [O] (optional): dW[o,h,m] = sum_{b,d} (gout + gpool)[b,o,d] X_0[b,h,d] X_{k-1}[b,m,d] */
int rp_cin_bs_bwd_w_workspace_bytes(int64_t B, int O, size_t *bytes);
int rp_cin_bs_bwd_w(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *gout, const float *gpool,
                    int H, int M, int O, int D, float *dW, float *db, int64_t B, void *workspace, size_t workspace_bytes,
                    rp_stream_t stream);
/* first layer only (X_{k-1} = X_0, O <= 128): the same dW [O, H*H] / db through the symmetric pair form — the products
 * X_0[h] X_0[m] are formed once per (pair, contraction row) instead of once per channel, and dWs[o, pair] is ONE TN GEMM */
int rp_cin_pair_fits(int H, int O, int D); /* H <= 32, O <= 128, D in {32, 64} */
/* forward of the same layer as ONE GEMM over the pair products: X_1[b,o,d] = bias[o] + sum_p Ws[o,p] X_0[b,h_p,d] X_0[b,m_p,d],
 * Ws[o,(h,m)] = W[o,h,m] + W[o,m,h] (h < m; W[o,h,h] on the diagonal), pairs row-major over the upper triangle.
 * wsp: Ws split into bf16 pieces (hi, mid, lo), [3][128][KP] with KP = 32*ceil(H(H+1)/2 / 32), zero padded.
 * out [B, O*D] or NULL, pooled [B, O] (sum over d) or NULL. */
int rp_cin_pair_fwd(const float *x0, int64_t ld0, const void *wsp, const float *bias, int H, int O, int D, float *out,
                    float *pooled, int64_t B, rp_stream_t stream);
/* dX_0 of the same layer (X_0 in both roles): T[p] = sum_o Ws[o,p] G[o], dX_0[h] = sum_{p=(h,m)|(m,h)} T[p] X_0[m].
 * wst: Ws^T as bf16 pieces [3][KPT][128], KPT = 128*ceil(H(H+1)/2 / 128), zero padded.  gout [B,O*D] / gpool [B,O] (packed)
 * as in rp_cin_bs_bwd_x.  lstart / lent (device int32): for pair tile t, half c (64 pairs) and field h the entries
 * lent[lstart[(2t+c)*H + h] .. lstart[(2t+c)*H + h + 1]) = (local pair row) | (other field) << 8 of that half's pairs
 * containing h, the diagonal pair listed twice.  dx rows [B, lddx]: the first H*D floats of each row are written —
 * accumulate != 0 (round 6): ADDED to what is there (the collapsed last layer's gradient of X_0, rp_cin_last_bwd_x: the sum of
 * the two without a pass of its own). */
int rp_cin_pair_bwd_x(const float *x0, int64_t ld0, const void *wst, const float *gout, const float *gpool,
                      const int32_t *lstart, const int32_t *lent, int H, int O, int D, float *dx, int64_t lddx, int64_t B,
                      int accumulate, rp_stream_t stream);
int rp_cin_pair_bwd_w_workspace_bytes(int64_t B, int H, int O, size_t *bytes);
int rp_cin_pair_bwd_w(const float *x0, int64_t ld0, const float *gout, const float *gpool, int H, int O, int D, float *dW,
                      float *db, int64_t B, void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- K6 (last layer): the collapsed final CIN layer ------------------------------------------------------
 * replaces interaction.py:157-171 for the LAST layer: with no activation and linear pooling + fc behind it, it
 * enters the logit only as  p[b] = sum_d sum_{h,m} V[h,m] X_0[b,h,d] X_{L-1}[b,m,d],  V = sum_o c[o] W_L[o].
 * x0 [B, ld0] holds H rows of D floats per sample, xp [B, ldp] M rows of D floats; vt = V^T zero-padded to [M, 32].
 * bwd_x: dx0[b,h,:] = g[b] sum_m V[h,m] Xp[b,m,:], dxp[b,m,:] = g[b] sum_h V[h,m] X0[b,h,:];  bwd_v: dV [H, M].
 * Limits: H <= 32, D <= 64 (rp_cin_last_fits). */
int rp_cin_last_fits(int H, int M, int D);
int rp_cin_last_fwd(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *vt, int H, int M, int D,
                    float *pooled, int64_t B, rp_stream_t stream);
int rp_cin_last_bwd_x(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *vt, const float *g, int H,
                      int M, int D, float *dx0, int64_t ldd0, float *dxp, int64_t lddp, int64_t B, rp_stream_t stream);
int rp_cin_last_bwd_v_workspace_bytes(int64_t B, int H, int M, size_t *bytes);
int rp_cin_last_bwd_v(const float *x0, int64_t ld0, const float *xp, int64_t ldp, const float *g, int H, int M, int D,
                      float *dV, int64_t B, void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* The weight-space arithmetic around the pair kernels and the collapsed last layer (round 6, csrc/cin_head.hip) — what the host
 * side did with ~50 elementwise / index / matmul launches per step (interaction.py:157-171 has no counterpart: the reference
 * runs every layer at full width):
 *   rp_cin_pair_pieces      W [O, H, H] -> the symmetric pair weights Ws[o, (h <= m)] = W[o,h,m] + W[o,m,h] (W[o,h,h] on the
 *                           diagonal) as three bf16 pieces (round to nearest even, piece k of what the pieces before it left):
 *                           wsp [3][128][KP] (rp_cin_pair_fwd / _bwd_w; KP = pairs rounded up to 32) and / or wst [3][KPT][128]
 *                           (rp_cin_pair_bwd_x; KPT = pairs rounded up to 128); either may be NULL; zero padded.
 *   rp_cin_head_params_fwd  vt [M, 32] = V^T zero padded, V[h, m] = sum_o c[o] WL[o, h M + m];  vb[0] = sum_o c[o] bL[o]
 *                           (bL may be NULL: 0) — c = the slice of fc.weight that multiplies the last layer's pooling.
 *   rp_cin_head_params_bwd  dWL[o, j] = c[o] dV[j];  dbL[o] = Dscale sg[0] c[o];  dc[o] = sum_j WL[o, j] dV[j] + Dscale sg[0] bL[o]
 *                           (dV [H, M] from rp_cin_last_bwd_v, sg[0] = sum_b g[b], Dscale = the embedding width D).
 *   rp_add_scalars          out[i] += scale a[0] + (b0 ? b0[0] : 0) for i < n (the head's D vb + fc.bias onto the [B] logit).
 *   rp_sum_all              out[0] = sum_i x[i], fixed order (one workgroup). */
int rp_cin_pair_pieces(const float *W, int O, int H, void *wsp, void *wst, rp_stream_t stream);
int rp_cin_head_params_fwd(const float *WL, const float *bL, const float *c, int O, int H, int M, float *vt, float *vb,
                           rp_stream_t stream);
int rp_cin_head_params_bwd(const float *WL, const float *bL, const float *c, const float *dV, const float *sg, float Dscale,
                           int O, int H, int M, float *dWL, float *dbL, float *dc, rp_stream_t stream);
int rp_add_scalars(float *out, int64_t n, const float *a, float scale, const float *b0, rp_stream_t stream);
int rp_sum_all(const float *x, int64_t n, float *out, rp_stream_t stream);

/* ---- K7 (split form): the T x T core of the field self-attention; projections are rp_linear_fwd GEMMs ------
 * replaces attention.py:20-33,73-94 for one AutoInt layer once QKVR = X . [Wq|Wk|Wv|Wres]^T has been computed for
 * all B*T token rows (row-major [B*T, ldq], columns Q | K | V | R, each H*a wide; nproj = 3 without W_res, the
 * residual then being xres [B*T, ldr] = X itself).  Heads are the reference's RAW view of a sample's flat [T*H*a]
 * buffer.  out [B*T, H*a] = relu(softmax(Q K^T [/scale]) V + R); stats [B, H*T, 2] = per-row (max, sum) of the
 * softmax, consumed by the backward.  Backward writes dqkvr (same layout; the R block = ReLU-masked dout) and, when
 * nproj == 3, dxres.  Limits: a <= 16 and a sample's Q,K,V,dO within 64 KB of LDS (rp_attention_core_fits). */
int rp_attention_core_fits(int T, int H, int a);
int rp_attention_core_fwd(const float *qkvr, int64_t ldq, int nproj, const float *xres, int64_t ldr, int T, int H,
                          int a, float scale, float *out, float *stats, int64_t B, rp_stream_t stream);
int rp_attention_core_bwd(const float *qkvr, int64_t ldq, int nproj, const float *out, const float *dout,
                          const float *stats, int T, int H, int a, float scale, float *dqkvr, int64_t lddq,
                          float *dxres, int64_t lddr, int64_t B, rp_stream_t stream);

/* ---- K7 (wide form): self-attention over few tokens with one wide head; the complement of rp_attention_core_* -------------
 * replaces attention.py:20-33,73-94 + a following torch.sum(., dim=1) where H == 1 and the head is wider than the core's 16
 * (AITM, multi_task/aitm.py:33,64-66: T = 2 tokens, a = 400, no W_res).  Operands as above with nproj == 3: qkv [B*T, ldq] with
 * columns Q | K | V (each a wide), xres [B*T, ldr] = the layer's input.  Per sample
 *   S[t,s] = q_t . k_s (/scale; scale == 0: none), P = softmax_s, O_t = sum_s P[t,s] v_s, Y_t = relu(O_t + xres_t)
 *   out = Y [B*T, a] (sum_tokens == 0) or sum_t Y_t [B, a] (sum_tokens != 0), contiguous.
 * Lanes run along a (one wave per sample, dwordx4 where a, the strides and the addresses are multiples of 16 bytes), the
 * T x T scores live in registers, no LDS, no workspace.  Backward: dout shaped like out; S, P and the ReLU mask are recomputed
 * from qkv and xres; writes dqkv [B*T, lddq] (Q | K | V) and dxres [B*T, lddr] = dY_t [Y_t > 0] (the residual's gradient; the
 * caller adds it to the dgrad GEMM's result).  One writer per element, no atomics: bit-identical from run to run.
 * Range (rp_attention_wide_fits): H == 1, 2 <= T <= 4, 1 <= a <= 65536; B >= 1. */
int rp_attention_wide_fits(int T, int H, int a);
int rp_attention_wide_fwd(const float *qkv, int64_t ldq, const float *xres, int64_t ldr, int T, int H, int a, float scale,
                          int sum_tokens, float *out, int64_t B, rp_stream_t stream);
int rp_attention_wide_bwd(const float *qkv, int64_t ldq, const float *xres, int64_t ldr, const float *dout, int T, int H,
                          int a, float scale, int sum_tokens, float *dqkv, int64_t lddq, float *dxres, int64_t lddr,
                          int64_t B, rp_stream_t stream);

/* dgrad with a fused row-scaled periodic addend (the DeepFM gather backward's FM term folded into dX):
 *   out[M,N] = a[M,K] . w[N,K]^T + row_scale[m] * row_add[m, n % 64]  for n < add_cols   (no bias / activation)
 * Only K <= 64 (multiple of 4), M % 128 == 0, N % 64 == 0, add_cols % 64 == 0, 16-byte aligned rows and a split-bf16
 * matmul mode; otherwise RP_ERR_UNSUPPORTED and the caller uses rp_linear_fwd + the sum_in path of the reduce. */
int rp_linear_fwd_rowadd(const float *a, int64_t lda, const float *w, int64_t ldw, float *out, int64_t ldo, int64_t M,
                         int N, int K, const float *row_scale, const float *row_add, int64_t ld_add, int add_cols,
                         rp_stream_t stream);

/* ---- stand-alone FM pooling on a [B,F,D] tensor -------------------------------------------------------
 * replaces layers/interaction.py:36-44 when the caller already holds the stacked embeddings (in DeepFM/FM the
 * gather kernel produces the term itself).  x[b] = F rows of D floats at x + b*ldb.
 *   out_sum [B] = product_sum_pooling, out_bi [B,D] = Bi_interaction_pooling (either may be NULL)
 *   backward: dx[b,f,:] = (g_sum[b] + g_bi[b,:]) * (sum_f x[b,f,:] - x[b,f,:])                             */
int rp_fm_pool_fwd(const float *x, int64_t ldb, int F, int D, float *out_sum, float *out_bi, int64_t B,
                   rp_stream_t stream);
int rp_fm_pool_bwd(const float *x, int64_t ldb, int F, int D, const float *g_sum, const float *g_bi, float *dx,
                   int64_t lddx, int64_t B, rp_stream_t stream);

/* ---- K9: BatchNorm1d of the MMOE towers ---------------------------------------------------------------
 * replaces nn.BatchNorm1d at multi_task/mmoe.py:54.  Training: batch mean / biased variance per column
 * (deterministic two-stage reductions, variance taken around the mean), y = (x-mean)*rstd*gamma+beta; the caller
 * updates the running statistics from mean/var.  Backward: dgamma = sum dy*xhat, dbeta = sum dy,
 * dx = gamma*rstd*(dy - mean(dy) - xhat*mean(dy*xhat)).  rp_batchnorm_apply(_bwd): given statistics (eval mode). */
int rp_batchnorm_workspace_bytes(int64_t M, int N, size_t *bytes);
int rp_batchnorm_train_fwd(const float *x, int64_t ldx, const float *gamma, const float *beta, float eps, float *y,
                           int64_t ldy, float *mean, float *var, float *rstd, int64_t M, int N, void *workspace,
                           size_t workspace_bytes, rp_stream_t stream);
int rp_batchnorm_train_bwd(const float *x, int64_t ldx, const float *dy, int64_t lddy, const float *mean,
                           const float *rstd, const float *gamma, float *dx, int64_t lddx, float *dgamma,
                           float *dbeta, int64_t M, int N, void *workspace, size_t workspace_bytes,
                           rp_stream_t stream);
int rp_batchnorm_apply(const float *x, int64_t ldx, const float *mean, const float *rstd, const float *gamma,
                       const float *beta, float *y, int64_t ldy, int64_t M, int N, rp_stream_t stream);
int rp_batchnorm_apply_bwd(const float *dy, int64_t lddy, const float *rstd, const float *gamma, float *dx,
                           int64_t lddx, int64_t M, int N, rp_stream_t stream);

/* ---- Dice activation (layers/activation.py:10-34: p = sigmoid(BatchNorm1d(x, affine=False, eps=1e-9, momentum=0.01)),
 * y = p x + (1 - p) alpha x).  The normalisation is rp_batchnorm_train_fwd / rp_batchnorm_apply with gamma = beta = NULL;
 * these are the gate around it on xhat = the normalised tensor (row-major, leading dimensions in floats):
 *   rp_dice_gate_fwd  y = x (alpha + s (1 - alpha)), s = sigmoid(xhat)
 *   rp_dice_gate_bwd  dx_direct = dy (alpha + s (1 - alpha)),  dxhat = dy x (1 - alpha) s (1 - s),  dal = dy x (1 - s)
 *                     (three packed [M, N] outputs; dalpha = column sums of dal: rp_batchnorm_colsum; dxhat goes on
 *                     through rp_batchnorm_train_bwd / rp_batchnorm_apply_bwd) */
int rp_dice_gate_fwd(const float *x, int64_t ldx, const float *xhat, int64_t ldh, const float *alpha, float *y, int64_t ldy,
                     int64_t M, int N, rp_stream_t stream);
int rp_dice_gate_bwd(const float *x, int64_t ldx, const float *xhat, int64_t ldh, const float *alpha, const float *dy,
                     int64_t lddy, float *dx_direct, float *dxhat, float *dal, int64_t M, int N, rp_stream_t stream);

/* building blocks of a BatchNorm1d whose batch statistics span several ranks (SyncBatchNorm1d of rec_pangu_amd/sharded.py;
 * mmoe.py:54 on the global batch).  The all-reduce between the stages is the caller's.
 *   rp_batchnorm_colsum     out[n] = sum_m x[m,n]  (center NULL)  |  sum_m (x[m,n] - center[n])^2  (center given)
 *   rp_batchnorm_bwd_sums   dbeta[n] = sum_m dy, dgamma[n] = sum_m dy * xhat  (xhat from the given mean / rstd)
 *   rp_batchnorm_bwd_apply  dx = gamma * rstd * (dy - mean_dy - xhat * mean_dyx) with the given (global) means
 * workspace: rp_batchnorm_workspace_bytes(M, N). */
/* nn.BatchNorm1d's running statistics of one training forward in ONE launch (mmoe.py:54 towers; torch/nn/modules/batchnorm.py):
 * num_batches_tracked (int64[1], may be NULL) += 1; running_x = (1 - m) running_x + m batch_x, the variance unbiased by
 * M / (M - 1); momentum < 0 = None: the cumulative average m = 1 / num_batches_tracked. */
int rp_batchnorm_update_running(const float *mean, const float *var, float *running_mean, float *running_var,
                                int64_t *num_batches_tracked, float momentum, int64_t M, int N, rp_stream_t stream);
int rp_batchnorm_colsum(const float *x, int64_t ldx, const float *center, float *out, int64_t M, int N, void *workspace,
                        size_t workspace_bytes, rp_stream_t stream);
int rp_batchnorm_bwd_sums(const float *x, int64_t ldx, const float *dy, int64_t lddy, const float *mean,
                          const float *rstd, float *dgamma, float *dbeta, int64_t M, int N, void *workspace,
                          size_t workspace_bytes, rp_stream_t stream);
int rp_batchnorm_bwd_apply(const float *x, int64_t ldx, const float *dy, int64_t lddy, const float *mean,
                           const float *rstd, const float *gamma, const float *mean_dy, const float *mean_dyx,
                           float *dx, int64_t lddx, int64_t M, int N, rp_stream_t stream);

/* ---- row-wise LayerNorm with a fused elementwise multiplier (csrc/layernorm.hip) --------------------------------------
 * replaces torch.nn.LayerNorm over the last dimension and the `net * mask` behind it in layers/interaction.py:269-283
 * (MaskBlock: _input_layer_norm, _layer_norm) and the stack + mean over parallel blocks of ranking/masknet.py:70-75.
 * x [M, ldx], gamma / beta [N], biased variance, two-pass statistics in registers (a wave64 per row up to N = 2048, a looped
 * path above: any N >= 1).  dwordx4 accesses where a pointer is 16-byte aligned and its leading dimension a multiple of 4.
 *   rp_layernorm_fwd   y = out_scale * ((gamma * (x - mu) * r + beta) [* mul])    (accumulate != 0: added to y)
 *                      mu = mean(x), r = 1 / sqrt(var(x) + eps) per row;  mul [M, ldmul] or NULL.
 *                      stats [M, 2] = (mu, r) per row: written (NULL: not kept), or READ when stats_given != 0 (several
 *                      LayerNorms over the same x: the parallel MaskBlocks).  Columns N .. N_pad-1 of y (N <= N_pad <= ldy)
 *                      are written as zeros.  out_scale / accumulate: the mean over K blocks is K launches with
 *                      out_scale = 1/K into one y, the first writing, the others adding, in the order they are issued.
 *   rp_layernorm_bwd   dn = dy_scale * dy [* mul],  g = gamma * dn,  nh = (x - mu) * r  from the saved stats:
 *                      dx (+)= r * (g - mean(g) - nh * mean(g * nh))    (accumulate != 0: added; columns N .. N_pad-1 zeros)
 *                      dmul = dy_scale * dy * (gamma * nh + beta)       (with mul only: the normalised row is recomputed,
 *                                                                        so the forward keeps x and mul, not their product)
 *                      dgamma[n] = sum_m dn * nh,  dbeta[n] = sum_m dn — per-wave partial rows in `workspace` over a
 *                      grid-stride walk of the rows, summed in a fixed order by a second launch (deterministic, no atomics).
 *                      workspace: rp_layernorm_bwd_workspace_bytes(N), independent of M. */
int rp_layernorm_fwd(const float *x, int64_t ldx, const float *gamma, const float *beta, float eps, const float *mul,
                     int64_t ldmul, float *y, int64_t ldy, int N_pad, float out_scale, int accumulate, float *stats,
                     int stats_given, int64_t M, int N, rp_stream_t stream);
int rp_layernorm_bwd_workspace_bytes(int N, size_t *bytes);
int rp_layernorm_bwd(const float *dy, int64_t lddy, float dy_scale, const float *x, int64_t ldx, const float *stats,
                     const float *gamma, const float *beta, const float *mul, int64_t ldmul, float *dx, int64_t lddx,
                     int N_pad, int accumulate, float *dmul, int64_t lddmul, float *dgamma, float *dbeta, int64_t M, int N,
                     void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- AOANet's generalized interaction layer without its outer product (csrc/gin.hip) ------------------------------------------
 * replaces GeneralizedInteraction.forward of ranking/aoanet.py:107-115, which builds the [B, P F, D, D] outer product of every
 * (input subspace, field) pair before contracting it.  Factorised, with M[o,h,d] = W[o,h,d] h[o,d]:
 *     T[b,o,p,h] = sum_d M[o,h,d] bi[b,p,d]     U[b,o,p,h] = sum_f alpha[p F + f, o] x0[b,f,h]     out[b,o,h] = sum_p T U
 * x0 [B, ldx0] (F D columns used: the embedding block of a wider row buffer), bi [B, ldbi] (P D columns; layer 0: x0 itself,
 * P = F), W [O, D, D], alpha [P F, O], h [O, D], out [B, ldo] (O D columns written), all fp32, row strides in floats, any
 * alignment.  Neither T, U nor anything else of size B O P D is written to global memory: the backward rebuilds them from x0,
 * bi and the parameters, a tile of samples at a time in LDS.  fp32 FMA on the vector ALU: no matrix-core mode applies.
 *   rp_gin_fits(F, P, O, D)   1 when the kernels cover the shape: D in {8, 16, 20, 32, 64}, 1 <= F, P <= 64, 1 <= O <= 16
 *                             (every such shape fits a tile of at least one sample in 144 KiB of LDS), else 0; outside it
 *                             rp_gin_fwd / rp_gin_bwd return RP_ERR_UNSUPPORTED.
 *   rp_gin_bwd   g = dout [B, lddo]:  dT = g U, dU = g T
 *                dx0[b,f,h] (+)= sum_{o,p} alpha[pF+f,o] dU     (accumulate != 0: added to what dx0 [B, lddx0] holds)
 *                dbi[b,p,d]  =  sum_{o,h} M[o,h,d] dT           (dbi [B, lddbi]; NULL only where bi is x0 itself — same
 *                                                                pointer, stride and P == F — and then ADDED into dx0's rows)
 *                dalpha[pF+f,o] = sum_{b,h} x0 dU,  dM[o,h,d] = sum_{b,p} dT bi,  dW = dM h,  dh[o,d] = sum_h dM W
 *                the three batch reductions through per-workgroup partials in `workspace` over a grid-stride walk of the
 *                sample tiles, summed in a fixed order by a second launch that also forms dW and dh from dM (no atomics:
 *                bit-identical from run to run).  workspace: rp_gin_bwd_workspace_bytes(F, P, O, D), independent of B. */
int rp_gin_fits(int F, int P, int O, int D);
int rp_gin_fwd(const float *x0, int64_t ldx0, const float *bi, int64_t ldbi, const float *W, const float *alpha,
               const float *h, float *out, int64_t ldo, int F, int P, int O, int D, int64_t B, rp_stream_t stream);
int rp_gin_bwd_workspace_bytes(int F, int P, int O, int D, size_t *bytes);
int rp_gin_bwd(const float *dout, int64_t lddo, const float *x0, int64_t ldx0, const float *bi, int64_t ldbi, const float *W,
               const float *alpha, const float *h, float *dx0, int64_t lddx0, int accumulate, float *dbi, int64_t lddbi,
               float *dW, float *dalpha, float *dh, int F, int P, int O, int D, int64_t B, void *workspace,
               size_t workspace_bytes, rp_stream_t stream);

/* ---- CCPM's conv + k-max-pooling + tanh stack as one launch each way (csrc/ccpm.hip) --------------------------------------------
 * replaces CCPM_ConvLayer.forward of ranking/ccpm.py:77-107: per layer l (C_in -> C_out channels, kernel (kh, 1), pooling size k)
 *     y[b,co,p,d] = bias[co] + sum_{ci,j} W[co,ci,j] xpad[b,ci,p+j,d]      (kh - 1 zero rows on either side: L_out = L_in + kh - 1)
 *     a[b,co,:,d] = tanh(the k largest of y[b,co,:,d], in their original order)              (L_in of the next layer = k)
 * No step mixes two embedding columns, so one thread runs the whole stack for one (b, d), its activations in LDS; nothing of
 * size B C L D is written to global memory, and the forward saves nothing but its output.  fp32 FMA on the vector ALU.
 * Selection: position i is kept iff #{j : y_j > y_i or (y_j == y_i and j < i)} < k — exact ties go to the LOWER index (torch's
 * topk leaves its tie order unspecified: the two may differ on exact ties, and only there).
 * x [B, ldx] (F D columns used, read in place: the embedding block of a wider row buffer), W[l] [C_out, C_in, kh(, 1)] and
 * bias[l] [C_out] contiguous, out [B, ldo] (C_last k_last D columns written, index c (k_last D) + j D + d: the reference's
 * flatten(conv_out, 1)), all fp32, row strides in floats, any alignment.  W / bias / dW / db: HOST arrays of n_layers device
 * pointers, channels / heights / ks: HOST arrays of n_layers ints (C_out, kh, k per layer); all are copied into the launch.
 *   rp_ccpm_fits   1 when the kernels cover the stack: 1 <= n_layers <= 3, every C_out in 1..4, kh in 1..8, 1 <= F <= 64,
 *                  1 <= D <= 65536, every L_out <= 64 and k in 1..L_out (L_out < k, where the reference's topk raises, is
 *                  refused), and the per-wave working set of either direction within 144 KiB of LDS; else 0, and
 *                  rp_ccpm_fwd / rp_ccpm_bwd return RP_ERR_UNSUPPORTED.
 *   rp_ccpm_bwd    from dout [B, lddo] and x alone (the forward and its selections are rebuilt per column): dx [B, lddx] (F D
 *                  columns written), dW[l], db[l].  The parameter gradients go through one partial per workgroup (at most 512
 *                  workgroups of 64 columns, walking the B D columns with the stride of the grid), summed in workgroup order by a
 *                  finishing launch: no floating-point atomics, bit-identical from run to run.
 *                  workspace: rp_ccpm_bwd_workspace_bytes(n_layers, channels, heights), independent of B. */
int rp_ccpm_fits(int F, int D, int n_layers, const int *channels, const int *heights, const int *ks);
int rp_ccpm_fwd(const float *x, int64_t ldx, const float *const *W, const float *const *bias, float *out, int64_t ldo, int F,
                int D, int n_layers, const int *channels, const int *heights, const int *ks, int64_t B, rp_stream_t stream);
int rp_ccpm_bwd_workspace_bytes(int n_layers, const int *channels, const int *heights, size_t *bytes);
int rp_ccpm_bwd(const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *const *W, const float *const *bias,
                float *dx, int64_t lddx, float *const *dW, float *const *db, int F, int D, int n_layers, const int *channels,
                const int *heights, const int *ks, int64_t B, void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- FiBiNet's SENET + bilinear interaction, written straight into the MLP's input (csrc/bilinear.hip) ----------------------------
 * replaces SENET_Layer + BilinearInteractionLayer (twice) + the two cats of ranking/fibinet.py:58-68 (= ranking/afm.py):
 *     Z = mean_d E,  A = relu(W2 relu(W1 Z))            (W1 [R, F], W2 [F, R], no biases; R = 0: no SENET, ONE branch)
 *     T[b,p,:] = (W_w(p) E[b,i,:]) * E[b,j,:]           pair p = (i, j), i < j, in itertools.combinations order, P = F (F - 1) / 2
 *     out[b, :] = T[b] (P D) | A_i A_j T[b] (P D, only with R > 0) | dense (n_dense)
 * The second branch is the reference's bilinear layer on V = E * A: a per-(sample, pair) scalar times the first, so the
 * matrix-vector product is formed once and V never.  fp32 FMA on the vector ALU (the forward is bound by what it writes).
 * x [B, ldx]: F D embedding columns, then n_dense dense columns, read in place; out [B, ldo]: only the columns above are
 * written; all fp32, row strides in floats, any alignment.  type: which pairs share a matrix; W: DEVICE array of NW device
 * pointers to contiguous [D, D] matrices (nn.Linear layout: W[d_out, d_in]), NW = 1 / F / P; wmap: DEVICE array of P ints,
 * the matrix of pair p (0 / i / p for the three types; values are clamped to 0 .. NW - 1).
 *   rp_bilinear_fits   1 for 2 <= F <= 40, D in {8, 16, 32, 64}, 0 <= R <= F and a known type; else 0, and the entry points
 *                      return RP_ERR_UNSUPPORTED.
 *   rp_bilinear_bwd    from dout [B, lddo] and x alone (A, U and T are rebuilt): dx [B, lddx], F D columns written (or added
 *                      to, accumulate != 0) — the bilinear and the SENET contributions summed; dW [NW, D, D] contiguous (a
 *                      matrix no pair uses gets zeros), dW1 [R, F], dW2 [F, R].  A sample-major launch (dx, per-workgroup
 *                      SENET partials), a pair-major launch (per (pair, batch slice) partials of dW) and a finishing launch
 *                      that sums slices, then the pairs of a matrix, then the SENET partials, all in a fixed order: no
 *                      floating-point atomics, bit-identical from run to run.  The batch is walked in chunks of 16384 samples
 *                      (two launches each), so the workspace — rp_bilinear_bwd_workspace_bytes(F, D, R, type) — is independent
 *                      of B. */
#define RP_BILINEAR_ALL 0         /* "field_all": one matrix */
#define RP_BILINEAR_EACH 1        /* "field_each": matrix i for the pairs (i, .) */
#define RP_BILINEAR_INTERACTION 2 /* "field_interaction": one matrix per pair */
int rp_bilinear_fits(int F, int D, int R, int type);
int rp_bilinear_fwd(const float *x, int64_t ldx, const float *W1, const float *W2, const float *const *W, const int *wmap,
                    float *out, int64_t ldo, int F, int D, int R, int type, int n_dense, int64_t B, rp_stream_t stream);
int rp_bilinear_bwd_workspace_bytes(int F, int D, int R, int type, size_t *bytes);
int rp_bilinear_bwd(const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *W1, const float *W2,
                    const float *const *W, const int *wmap, float *dx, int64_t lddx, int accumulate, float *dW, float *dW1,
                    float *dW2, int F, int D, int R, int type, int n_dense, int64_t B, void *workspace, size_t workspace_bytes,
                    rp_stream_t stream);

/* ---- the narrow tail of the MLP as one launch each way (layers/deep.py:62-72 with hidden_units [.., 64, 64], output_dim 1:
 * DeepFM's dnn.net.{2,4,6}) --------------------------------------------------------------------------------------------
 *   hin [M, 64] (a ReLU output) -> [Linear 64x64 + ReLU] x n_hidden (1..3) -> Linear 64 -> 1 = logit [M]
 * rp_mlp_tail_fwd   W_hidden[l] [64 out, 64 in] (ldw[l] floats per row), b_hidden[l] [64] or NULL, h_out[l] [M, 64]: the
 *                   hidden outputs, saved for the backward; w_out [64], b_out [1] or NULL
 * rp_mlp_tail_bwd   dz [M] -> dhin [M, lddh] (already masked by hin > 0) and `grads` = dW_0 | .. | db_0 | .. | dw_out | db_out
 *                   packed (n_hidden*4096 + n_hidden*64 + 64 + 1 floats); acts[0] = hin (ldact0), acts[l] = h_out[l-1];
 *                   per-workgroup partials through `workspace`, summed in a fixed order (deterministic)
 * Split-bf16 six-product MFMAs (fp32-faithful) in every precision mode except RP_MATMUL_FP32 (callers compose the plain
 * entry points there).  rp_mlp_tail_fits: width 64, 1..3 hidden layers, row strides multiples of 4 floats. */
int rp_mlp_tail_fits(int n_hidden, int width, int64_t ldin);
int rp_mlp_tail_fwd(const float *hin, int64_t ldin, int n_hidden, const float *const *W_hidden, const int64_t *ldw,
                    const float *const *b_hidden, float *const *h_out, const float *w_out, const float *b_out, float *logit,
                    int64_t M, rp_stream_t stream);
int rp_mlp_tail_bwd_workspace_bytes(int64_t M, int n_hidden, size_t *bytes);
int rp_mlp_tail_bwd(const float *dz, int n_hidden, const float *const *W_hidden, const int64_t *ldw, const float *const *acts,
                    int64_t ldact0, const float *w_out, float *dhin, int64_t lddh, float *grads, int64_t M, void *workspace,
                    size_t workspace_bytes, rp_stream_t stream);
/* the same in two separately issued parts: parts = 1 the per-workgroup launch (dhin + partial sums into the workspace),
 * 2 = the second stage (workspace -> grads), 3 = both (= rp_mlp_tail_bwd).  The second stage reads only the workspace, so
 * a captured step issues it beside the launches that follow the first one. */
int rp_mlp_tail_bwd_parts(const float *dz, int n_hidden, const float *const *W_hidden, const int64_t *ldw,
                          const float *const *acts, int64_t ldact0, const float *w_out, float *dhin, int64_t lddh, float *grads,
                          int64_t M, void *workspace, size_t workspace_bytes, int parts, rp_stream_t stream);

/* The tail with the model's loss head inside (ranking/deepfm.py:61-66 on top of layers/deep.py:61-84; three launches of a
 * DeepFM step in one each way).  Forward: pred [M] = sigmoid(addends[0][m] + .. + tail logit) (0..3 other addends, summed in
 * that order, the tail's logit last), partial [rp_mlp_tail_loss_partials(M)] = per-workgroup sums of the BCE terms of
 * (pred + p_eps, label), logs clamped at -100: rp_loss_finish(partial, n, weight / M, loss) gives the mean loss — term for
 * term rp_sigmoid_bce_fwd's arithmetic (pred is bit-identical to the separate launches; the loss differs by the order of
 * its sum).  Backward: the logit's gradient is formed per row from (pred, label, gloss[0] * weight / M) — rp_sigmoid_bce_bwd
 * bit for bit — and written to dz_out [M] (NULL: not) for the other addends; everything else as rp_mlp_tail_bwd_parts. */
int rp_mlp_tail_loss_partials(int64_t M);
int rp_mlp_tail_fwd_bce(const float *hin, int64_t ldin, int n_hidden, const float *const *W_hidden, const int64_t *ldw,
                        const float *const *b_hidden, float *const *h_out, const float *w_out, const float *b_out,
                        const float *const *addends, int n_addends, const float *label, float p_eps, float *pred,
                        float *partial, int64_t M, rp_stream_t stream);
int rp_mlp_tail_bwd_bce(const float *pred, const float *label, const float *gloss, float p_eps, float weight, float *dz_out,
                        int n_hidden, const float *const *W_hidden, const int64_t *ldw, const float *const *acts,
                        int64_t ldact0, const float *w_out, float *dhin, int64_t lddh, float *grads, int64_t M,
                        void *workspace, size_t workspace_bytes, int parts, rp_stream_t stream);

/* ---- Dropout (layers/deep.py:66-68 inside the MLP chain; the multi-task towers, mmoe.py:55) -------------------------
 * y = x * keep / (1 - p), keep ~ Bernoulli(1 - p) from Philox4x32-10(counter = (element group, offset), key = seed): a
 * pure function of (seed, offset, element index).  mask: uint8 [M*N] (1 = kept), saved for the backward
 * dx = dy * keep / (1 - p).  One call consumes ONE offset value (the host advances its generator by one per call). */
int rp_dropout_fwd(const float *x, int64_t ldx, float *y, int64_t ldy, uint8_t *mask, int64_t M, int N, float p,
                   uint64_t seed, uint64_t offset, rp_stream_t stream);
/* the same with offset = *offset_dev + offset_delta read on the device: what a captured step records (frozen launch
 * arguments): offset_dev holds the generator offset of the step's start and is advanced at the step's end with
 * rp_counter_add_u64, so a replay draws the masks the eager loop would draw at that point of the generator's stream */
int rp_dropout_fwd_dev(const float *x, int64_t ldx, float *y, int64_t ldy, uint8_t *mask, int64_t M, int N, float p,
                       uint64_t seed, uint64_t offset_delta, const uint64_t *offset_dev, rp_stream_t stream);
int rp_counter_add_u64(uint64_t *counter, uint64_t delta, rp_stream_t stream);
int rp_dropout_bwd(const float *dy, int64_t lddy, const uint8_t *mask, float *dx, int64_t lddx, int64_t M, int N, float p,
                   rp_stream_t stream);

/* ---- K10: logit sum + sigmoid + BCE(mean) ---------------------------------------------------
 * replaces ranking/deepfm.py:61-63 (sigmoid + torch.nn.BCELoss) and multi_task/mmoe.py:127.
 *   z = sum_i z_ptrs[i][b] (n_addends <= 4; pass apply_sigmoid=0 when z is already a probability)
 *   pred[b] = sigmoid(z);  loss = weight * mean_b BCE(pred + p_eps, label), logs clamped at -100
 *   partial: float[rp_loss_partials(B)] workspace;  loss: device float[1] (written unless NULL) */
int rp_loss_partials(int64_t B);
int rp_sigmoid_bce_fwd(const float *const *z_ptrs, int n_addends, int apply_sigmoid, const float *label,
                       int64_t B, float p_eps, float weight, float *pred, float *partial, float *loss,
                       rp_stream_t stream);
/* rp_sigmoid_bce_fwd with loss[0] += instead of = : the second .. last task of a multi-task loss (mmoe.py:127: the sum of the
 * tasks' weighted means, added in task order like the reference's python sum) */
int rp_sigmoid_bce_fwd_accum(const float *const *z_ptrs, int n_addends, int apply_sigmoid, const float *label,
                             int64_t B, float p_eps, float weight, float *pred, float *partial, float *loss,
                             rp_stream_t stream);
/* loss[0] = scale * sum(partial[0..n)), fixed order (the second stage of rp_sigmoid_bce_fwd; also ends rp_mlp_tail_fwd_bce) */
int rp_loss_finish(const float *partial, int n, float scale, float *loss, rp_stream_t stream);
/* dz[b] = gloss[0] * weight/B * dBCE/dp * (apply_sigmoid ? p(1-p) : 1) */
int rp_sigmoid_bce_bwd(const float *pred, const float *label, const float *gloss, int64_t B, float p_eps,
                       float weight, int apply_sigmoid, float *dz, rp_stream_t stream);

/* ---- epoch metrics: binary ROC-AUC as an exact rational + the float64 log-loss sum (csrc/metrics.hip) ----------------------
 * replaces the .cpu() of every prediction + sklearn's roc_auc_score / log_loss at the end of model_pipeline.py's loops.
 *   pred, label  float[n] on the device, 1 <= n < 2^31 - 1
 *   two_u        sum over the positives (label == 1) of #negatives (label == 0) with a smaller prediction
 *                + #negatives with a smaller or equal one: AUC = two_u / (2 P N), ties counted as halves, exact integers
 *   P, N         counts of label == 1 / label == 0
 *   unsupported  elements whose prediction is not finite or whose label is neither 0 nor 1 (the caller then takes its
 *                host path: the other fields are computed all the same but mean nothing)
 *   logloss_sum  sum of -(label == 1 ? log q : log(1 - q)), q = min(max((double)pred, eps), 1 - eps), in float64, added in
 *                a fixed order (no atomics): two calls give the same bits.  Divide by n for the mean.
 * flags: RP_METRIC_AUC | RP_METRIC_LOGLOSS, what to compute (the counts always are; log-loss alone skips the sort and
 * leaves two_u = 0).  RP_METRICS_STAGE_* bits, for measurements only: issue just those launches (none = all of them);
 * stages issued one call after the other over the same workspace give the result of one whole call.
 * Kernel launches only, on `stream`; result is device memory (8-byte aligned) — one 40-byte copy brings everything back.
 * Nothing is allocated: workspace from rp_metrics_workspace_bytes(n) (~21 n bytes).  pred, label, result and the workspace
 * must not overlap. */
typedef struct {
    int64_t two_u, P, N, unsupported;
    double logloss_sum;
} rp_binary_metrics_result;
#define RP_METRIC_AUC 1
#define RP_METRIC_LOGLOSS 2
#define RP_METRICS_STAGE_KEY 0x100
#define RP_METRICS_STAGE_SORT 0x200
#define RP_METRICS_STAGE_TILE_SUMS 0x400
#define RP_METRICS_STAGE_TILE_SCAN 0x800
#define RP_METRICS_STAGE_GROUP_NEG 0x1000
#define RP_METRICS_STAGE_RANK 0x2000
#define RP_METRICS_STAGE_FINISH 0x4000
#define RP_METRICS_STAGE_ALL 0x7F00
int rp_metrics_workspace_bytes(int64_t n, size_t *bytes);
int rp_binary_metrics(void *workspace, size_t workspace_bytes, const float *pred, const float *label, int64_t n, double eps,
                      int flags, rp_binary_metrics_result *result, rp_stream_t stream);

/* ---- two-task loss heads that couple the tasks ---------------------------------------------------------------------------
 * replaces multi_task/essm.py:69-75 and multi_task/aitm.py:84-100 (and the two sigmoids in front of them).
 *   p_i = sigmoid(z_i) (apply_sigmoid) or z_i;  BCE = mean over the batch, ATen's form (logs clamped at -100)
 *   RP_PAIR_ESSM: loss = BCE(p1 p2, y2) + coef BCE(p1, y1)
 *   RP_PAIR_AITM: loss = BCE(p1, y1) + BCE(p2, y2) + coef sum_b max(p2 - p1, 0)       (a sum, not a mean)
 * p1, p2: float[B] out;  partial: float[3 * rp_loss_partials(B)] workspace (per-workgroup sums of the two BCE terms and of the
 * constraint, added in a fixed order by a one-block finish that scales them only then: no atomics);  loss: device float[1].
 * Backward: dz_i = gloss[0] dloss/dz_i from (p1, p2, y1, y2); ESSM with q = p1 p2: dp1 = dq p2 + coef bce'(p1, y1), dp2 = dq p1;
 * AITM: dp2 = bce'(p2, y2) + coef s, dp1 = bce'(p1, y1) - coef s with s = 1 / 0 / 0.5 for p2 > / < / == p1 (ATen's maximum);
 * bce'(p, y) = (p - y) / max((1 - p) p, 1e-12) / B. */
#define RP_PAIR_ESSM 0
#define RP_PAIR_AITM 1
int rp_pair_loss_fwd(const float *z1, const float *z2, const float *y1, const float *y2, int64_t B, int mode, float coef,
                     int apply_sigmoid, float *p1, float *p2, float *partial, float *loss, rp_stream_t stream);
int rp_pair_loss_bwd(const float *p1, const float *p2, const float *y1, const float *y2, const float *gloss, int64_t B,
                     int mode, float coef, int apply_sigmoid, float *dz1, float *dz2, rp_stream_t stream);

/* ---- AFN's logarithmic transformation layer + both BatchNorms (csrc/lognet.hip) --------------------------------------------
 * replaces ranking/afn.py:93-102:  x = log(max(|e|, 1e-5f));  y = BN1(x), channel = field, statistics over (b, d);
 * z[b,l,d] = sum_f W[l,f] y[b,f,d];  c = exp(z);  out = BN2(c), channel = neuron.
 *   x    [B, ldx >= F D]  the gather's rows, read in place;  W [L, F];  z [B, L D] (written, saved for the backward);
 *   out  [B, ldo >= L D]  L D columns written.  x, y and c never exist in global memory.
 *   rp_lognet_fits   1 for 1 <= F <= 64, 1 <= D <= 256, 1 <= L <= 8 (the shapes whose kernels use no scratch); else 0, and the
 *                    entry points return RP_ERR_UNSUPPORTED.  B D < 2^31.
 *   rp_lognet_plan   the partial workgroups (<= 512) of every reduction over the B D (sample, column) pairs and their run.
 *   train != 0       batch statistics: mean1 / var1 [F] and mean2 / var2 [L] (biased) are WRITTEN (two-stage, fixed order,
 *                    per-workgroup (mean, M2) pairs merged: centred); 5 launches.  The running buffers are the caller's
 *                    (rp_batchnorm_update_running with M = B D).
 *   train == 0       the four vectors are read (running statistics); 1 launch.
 *   rp_lognet_bwd    from dout [B, lddo], x and z, with the statistics the forward used: dx [B, lddx] (F D columns written:
 *                    BN1'(W^T dz) / e where |e| >= 1e-5f, exactly 0 elsewhere), dW [L, F], dgamma1 / dbeta1 [F], dgamma2 /
 *                    dbeta2 [L]; train == 0: the statistics are constants.  5 launches, every sum two-stage in a fixed order;
 *                    workspace rp_lognet_workspace_bytes(F, L), independent of B. */
int rp_lognet_fits(int F, int D, int L);
int rp_lognet_plan(int64_t B, int D, int *nblk, int64_t *chunk);
int rp_lognet_workspace_bytes(int F, int L, size_t *bytes);
int rp_lognet_fwd(const float *x, int64_t ldx, const float *W, const float *gamma1, const float *beta1, float *mean1,
                  float *var1, float eps1, const float *gamma2, const float *beta2, float *mean2, float *var2, float eps2,
                  float *z, float *out, int64_t ldo, int64_t B, int F, int D, int L, int train, void *workspace,
                  size_t workspace_bytes, rp_stream_t stream);
int rp_lognet_bwd(const float *dout, int64_t lddo, const float *x, int64_t ldx, const float *z, const float *W,
                  const float *gamma1, const float *beta1, const float *mean1, const float *var1, float eps1,
                  const float *gamma2, const float *mean2, const float *var2, float eps2, float *dx, int64_t lddx, float *dW,
                  float *dgamma1, float *dbeta1, float *dgamma2, float *dbeta2, int64_t B, int F, int D, int L, int train,
                  void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* AFN's ensemble head (afn.py:81, nn.Linear(2, 1) over cat[a, d]):  z[b] = w[0] a[b] + w[1] d[b] + bias[0], and its backward
 * da = w[0] dz, dd = w[1] dz, dw [2] = (sum dz a, sum dz d), dbias [1] = sum dz (per-workgroup partials + a fixed-order
 * finish; partial: float[rp_pair_fc_partials(B)]). */
int rp_pair_fc_partials(int64_t B);
int rp_pair_fc_fwd(const float *a, const float *d, const float *w, const float *bias, float *z, int64_t B, rp_stream_t stream);
int rp_pair_fc_bwd(const float *dz, const float *a, const float *d, const float *w, float *da, float *dd, float *dw,
                   float *dbias, float *partial, int64_t B, rp_stream_t stream);

/* ---- multi-id ("bag") lookups with pooling: the CSR / segmented embedding gather + sum-pool of the north star ----------
 * replaces EmbeddingLayer.forward(X, name="<col>_seq") (rec_pangu/models/layers/embedding.py:64-71: [B, L] ids ->
 * [B, L, D]) FOLLOWED BY MaskedSumPooling (layers/sequence.py:38-59: sum over dim 1) or MaskedAveragePooling
 * (layers/sequence.py:13-36: sum / (count of non-zero ELEMENTS per (b, d) + 1e-16)) — the [B, L, D] tensor never exists.
 *   ids: int64; dense bags: offsets = NULL, bag b = ids[b*L .. b*L+L); CSR bags: offsets int64 [B+1] into ids.
 *   The table is rows [row_base, row_base + row_count) of the arena; an id outside [0, row_count) sets *err_flag and
 *   reads row 0 (the reference raises IndexError).  mode 0 = sum, 1 = masked average.
 *   out [B, ldo >= D]; inv_out [B, D] (mode 1, for the backward: 1 / (count + 1e-16)) or NULL;
 *   bag_out int32 [nnz] (CSR, for the backward: the bag of every id) or NULL.
 * rp_embed_pool_bwd: grad_arena[row] (+)= sum over the ids p of that row of g[bag(p), :] (* scale[bag(p), :]), from the
 *   (arena row, flat id position) pairs sorted by row (rp_embed_keys with F = 1 over the flat ids, rp_sort_pairs_i32);
 *   bag(p) = bag_of[p], or p / L when bag_of is NULL.  Deterministic (the segmented reduction of rp_embed_grad_reduce,
 *   same workspace): a padding id present in every bag is one long run like any hot row.
 * rp_seq_pool_fwd / _bwd: the same two poolings on an explicit, contiguous [B, L, D] tensor (the drop-in modules). */
int rp_embed_gather_pool_fwd(const float *arena, int64_t row_base, int64_t row_count, const int64_t *ids,
                             const int64_t *offsets, int64_t L, int64_t B, int D, int mode, float *out, int64_t ldo,
                             float *inv_out, int32_t *bag_out, int32_t *err_flag, rp_stream_t stream);
int rp_embed_pool_bwd(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int D, const float *g, int64_t ldg,
                      const float *scale, const int32_t *bag_of, int64_t L, float *grad_arena, int accumulate,
                      void *workspace, size_t workspace_bytes, rp_stream_t stream);
int rp_seq_pool_fwd(const float *e, int64_t B, int64_t L, int D, int mode, float *out, float *inv_out, rp_stream_t stream);
int rp_seq_pool_bwd(const float *g, const float *inv, int64_t B, int64_t L, int D, float *de, rp_stream_t stream);

/* ---- sequence recall: the full-softmax loss head and the masked history mean (csrc/softmax_ce.hip, csrc/pool.hip) --------
 * rp_softmax_ce_fwd / _bwd replace SequenceBaseModel.calculate_loss (rec_pangu/models/base_model.py:124-138:
 *   scores = user_emb @ item_emb.weight.T  [B, V];  loss = CrossEntropyLoss()(scores, target)) and its autograd, which keeps
 * the logits, the softmax and their gradient — three [B, V] tensors.  Here none exists:
 *   U [B, ldu >= D] fp32, E [V, D] fp32 contiguous, target int64 [B] in [0, V), s[b, v] = sum_d U[b, d] E[v, d]
 *   fwd:  lse[b] = log sum_v exp(s[b, v]) (float[B]),  loss[0] = (1/B) sum_b (lse[b] - s[b, target[b]])
 *   bwd:  with p'[b, v] = exp(s[b, v] - lse[b]) - [v == target[b]] and g = gloss[0] (device float):
 *         dU[b, :] = (g/B) sum_v p'[b, v] E[v, :]   ([B, lddu >= D], or NULL)
 *         dE[v, :] = (g/B) sum_b p'[b, v] U[b, :]   ([V, D] contiguous, or NULL)
 * A target outside [0, V) sets *err_flag and counts as item 0 (the reference raises IndexError).  Score tiles are formed on
 * the bf16 matrix core from split-bf16 operands (product count: rp_set_matmul_precision; the automatic mode runs the
 * fp32-faithful six); no floating-point atomics, results are bit-identical from run to run.  1 <= D <= max_d of
 * rp_softmax_ce_geometry (128), RP_ERR_ARG above.  workspace: rp_softmax_ce_workspace_bytes(B, V, D) bytes, 16-byte aligned,
 * the same for both calls; it holds one (max, sum) pair per (row, split of V), the dU slab of each split and the loss
 * partials — nothing of size B x V.
 * rp_softmax_ce_geometry: tb = rows of U per workgroup, tv = rows of E per tile, max_d, slices = lanes per row of the
 * finishing merge (slice q merges the splits q, q + slices, ... in ascending order).  rp_softmax_ce_splits: the number of
 * splits of V and the tiles of E in each (the last may hold fewer) for a batch of B rows.
 * rp_hist_mean_fwd / _bwd replace the lookup, mask product and mean of rec_pangu/models/sequence/yotubednn.py:34-36:
 *   out[b, :] = (1/L) sum_l mask[b, l] E[hist[b, l], :]   (hist int64 [B, L], mask float [B, L]; the divisor is L)
 * without the [B, L, D] tensor; an id outside [0, V) sets *err_flag and reads row 0.  The backward ADDS
 * (mask[b, l] / L) g[b, :] into dE[hist[b, l], :] for every position whose id is not 0 (the table is
 * nn.Embedding(padding_idx=0): row 0 takes no gradient from lookups whatever the mask says), from the (id, flat position)
 * pairs sorted by id (rp_sort_pairs_i32 over the flat int32 ids); one writer per row, a fixed order. */
int rp_softmax_ce_geometry(int *tb, int *tv, int *max_d, int *slices);
int rp_softmax_ce_splits(int64_t B, int64_t V, int *nsplit, int64_t *tiles_per_split);
int rp_softmax_ce_workspace_bytes(int64_t B, int64_t V, int D, size_t *bytes);
int rp_softmax_ce_fwd(const float *U, int64_t ldu, const float *E, const int64_t *target, int64_t B, int64_t V, int D,
                      float *lse, float *loss, int32_t *err_flag, void *workspace, size_t workspace_bytes,
                      rp_stream_t stream);
int rp_softmax_ce_bwd(const float *U, int64_t ldu, const float *E, const int64_t *target, const float *lse,
                      const float *gloss, int64_t B, int64_t V, int D, float *dU, int64_t lddu, float *dE, void *workspace,
                      size_t workspace_bytes, rp_stream_t stream);
int rp_hist_mean_fwd(const float *E, int64_t V, int D, const int64_t *hist, const float *mask, int64_t B, int64_t L,
                     float *out, int64_t ldo, int32_t *err_flag, rp_stream_t stream);
int rp_hist_mean_bwd(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int64_t L, int D, int64_t V,
                     const float *mask, const float *g, int64_t ldg, float *dE, rp_stream_t stream);

/* ---- K11: fused Adam (torch.optim.Adam single-tensor operation order) -----------------------
 * replaces trainer.py:75 + model_pipeline.py:57-58 (optimizer.step(); model.zero_grad()).
 * n_tensors <= RP_MAX_FIELDS per call; zero_grad=1 also clears g (the fused zero_grad).
 * lr, betas and eps are DOUBLES, like the python floats torch.optim.Adam computes its bias corrections from (a float
 * beta2 = 0.999f shifts 1 - beta2^t by 5e-6 relative at t ~ 600).
 * The second-moment arrays (`v_ptrs`, and `v` of the lazy entry points below) hold s = sqrt(v), not v: Adam only uses
 * sqrt(v), and a zero-gradient step is then s *= sqrt(b2) (one multiply, no transcendental) — chosen per element on
 * g == 0 by the one update function all these kernels share, so dense and lazy execution stay bit-identical.  The
 * host side squares s when it exports torch.optim.Adam-style state (rec_pangu_amd/optim.py).  */
int rp_adam_step(float *const *p_ptrs, float *const *g_ptrs, float *const *m_ptrs, float *const *v_ptrs,
                 const int64_t *sizes, int n_tensors, double lr, double beta1, double beta2, double eps,
                 int64_t step, int zero_grad, const float *step_scalars, const int32_t *t_dev, rp_stream_t stream);
/* DEVICE-RESIDENT STEP COUNTERS (hipGraph replays freeze every launch argument at capture, so the step number cannot be
 * one).  Wherever an entry point of this section takes `t_dev` (device int32[1] = number of COMPLETED optimizer steps,
 * NULL = use the host arguments), the kernel reads the step from it: rp_adam_step applies step *t_dev + 1 with the
 * scalars step_scalars[*t_dev + 1] (the float2 table of rp_adam_step_scalars rows indexed by step; lr / step arguments
 * ignored), rp_lazy_adam_rows replays to *t_dev (real_step: applies *t_dev + 1), rp_lazy_adam_cf_table builds the table
 * for t_end = *t_dev (a fixed-size window of the youngest stamps: consecutive replays keep it complete).  rp_counter_add advances a
 * counter on the stream.  rec_pangu_amd/graph_step.py captures fwd + bwd + optimizer on top of these. */
int rp_counter_add(int32_t *counter, int32_t delta, rp_stream_t stream);
/* the same for 1..8 distinct counters in one launch (counters: host array of device pointers) */
int rp_counters_add(int32_t *const *counters, int n, int32_t delta, rp_stream_t stream);

/* ---- exact LAZY dense Adam for arena rows -----------------------------------------------------
 * Same semantics as rp_adam_step over the whole arena (trainer.py:75: DENSE Adam, every row every step), but a
 * row's zero-gradient steps are replayed in registers when the row is next needed instead of being streamed
 * through HBM every step.  last[row] (int32, 0 = never updated) is the step the stored (p,m,v) are current at;
 * step_scalars is a device float2 table indexed by step: {A_t, B_t} from rp_adam_step_scalars (the eps given
 * there is the one that counts for the serial replay).  The serial replay runs the dense kernel's update function with
 * g = 0: bit-identical results.
 *   rp_embed_keys       arena-row keys of a batch (same check/flag/clamp as the gather) — needed before the gather
 *   rp_lazy_adam_rows   for every UNIQUE row of `sorted_keys` (sorted; duplicates skipped): replay steps
 *                       last+1 .. t_target(-1); if real_step also apply step t_target with g = grad row
 *                       (and clear it if zero_grad); last[row] = t_target
 *   rp_lazy_adam_flush  replay every row up to t_target (before a checkpoint / state_dict / eval of raw tables)
 * Any D >= 1.  Pure replays (real_step = 0) and the flush of rows wider than 16 floats run ONE ROW PER WAVE (the chain
 * length differs per row: side by side in a wave every row would wait for the longest), candidates strided over the
 * waves so that every wave sees the same mix of tables; the real step and narrow rows (D = 1: the LR_Layer's tables)
 * use 16-byte vector lanes when D % 4 == 0 and the arenas are 16-byte aligned, scalar lanes otherwise. */
int rp_embed_keys(const int64_t *row_base, const int64_t *row_count, const int64_t *const *idx_ptrs, int F, int64_t B,
                  int32_t *keys_out, int32_t *err_flag, rp_stream_t stream);
int rp_adam_step_scalars(double lr, double beta1, double beta2, double eps, int64_t step, float *sa,
                         float *sb);
/* the same for n consecutive steps step0 .. step0 + n - 1: out[2 i], out[2 i + 1] = {A, B} of step step0 + i (HOST array) */
int rp_adam_step_scalars_range(double lr, double beta1, double beta2, double eps, int64_t step0, int64_t n, float *out); /* {A_t, B_t} = {1/sqrt(1-b2^t), eps} / (-lr/(1-b1^t)), computed in double: the update
                                      * is p += m * rcp(s * A_t + B_t) (s = sqrt(v)); lr = 0 gives (0, -inf) */
int rp_lazy_adam_rows(const int32_t *sorted_keys, int64_t n, int D, float *p, float *g, float *m, float *v,
                      int32_t *last, const float *step_scalars, int64_t t_target, int real_step, int zero_grad,
                      double beta1, double beta2, double eps, const float *cf_table, int64_t cf_from, const int32_t *t_dev,
                      rp_stream_t stream);
int rp_lazy_adam_flush(int64_t rows, int D, float *p, float *m, float *v, int32_t *last, const float *step_scalars,
                       int64_t t_target, double beta1, double beta2, double eps, const float *cf_table, int64_t cf_from,
                       rp_stream_t stream);
/* CLOSED-FORM replay (cf_table != NULL in the two entry points above; tolerance mode, NULL = the bit-exact serial
 * replay).  The k zero-gradient steps l+1 .. l+k of an element are  m b1^k,  s r^k  and
 *     p + m * sum_i w_i / (s a_i + eps),  w_i = -lr_{l+i}/(1-b1^{l+i}) b1^i,  a_i = r^i / sqrt(1-b2^{l+i}),  r = sqrt(b2);
 * every term is expanded around the w-weighted mean abar of the a_i:  q [N0 + y^2 N2 - y^3 N3 + y^4 N4],
 * q = 1/(s abar + eps), y = s q, N_n = sum_i w_i (a_i - abar)^n — uniformly convergent in s (|y (a_i - abar)| <=
 * |a_i/abar - 1|), relative truncation error of the summed update <= 9e-8 once l >= 256 at b2 = 0.999
 * (profiles/microbench/probes/closed_form_replay.py).  Steps up to `cf_from` are still replayed serially; steps cf_from+1 .. t cost one
 * reciprocal and ~10 fp32 operations per element whatever their number.  Here `eps` counts (it is the eps of the
 * expansion) and must be the one the step scalars were built with.
 *   rp_lazy_adam_cf_table  cf_table: `capacity` entries of 8 floats (abar, N0, N2, -N3, N4, b1^k, r^k, 0) with TWO index
 *                          meanings: the first five of entry l describe a replay that starts at stamp l (steps l+1 ..
 *                          t_end), cf_from <= l < t_end; the two powers of entry k belong to a replay of k steps.  Valid
 *                          for replays that END at t_end (rp_lazy_adam_rows(real_step=0, t_target=t_end), (real_step=1,
 *                          t_target=t_end+1), rp_lazy_adam_flush(t_target=t_end)).  Built on the device, in double:
 *                          built_to < 0 = a fresh buffer (the power columns and every stamp: O(t_end) once); otherwise
 *                          built_to = the t_end of the previous call on this buffer and only the stamps that were not
 *                          final then ( >= built_to - J, J = rp_lazy_adam_cf_terms) are rebuilt: O(1) per training step
 *                          whatever the step count.  With t_dev (consecutive graph replays) the window is the J + 4
 *                          youngest stamps below *t_dev.  ns_d: device double2 table indexed by step:
 *                          {-lr_j/(1-b1^j), 1/sqrt(1-b2^j)} (rows of steps already taken never change).
 *   rp_lazy_adam_cf_terms  number of leading terms that carry weight (b1^J < 1e-17) */
int rp_lazy_adam_cf_terms(double beta1, int *terms);
/* DEFERRED real step (opt-in execution mode of the same optimizer; no reference counterpart beyond trainer.py:75).
 * A row's real step needs only its own gradient row, which stays in the (dense) gradient arena: it can wait, like the
 * zero-gradient steps, until the row is next needed.  One launch per training step then does what the rows of the
 * incoming batch are owed — 8 rows of traffic per unique row instead of 6 (replay) + 8 (step).
 *   last[row] >= 0: as above.  last[row] < 0: (p,m,v) current through step l = -last-1 and g[row] = the gradient of
 *   step l+1, not applied yet.
 *   rp_lazy_adam_catchup  for every unique row of sorted_keys: a pending gradient whose step has been taken
 *                         (l+1 <= t_done) is applied with the scalars of step l+1 and its row cleared, then the
 *                         zero-gradient steps up to t_done (serial up to cf_from, closed form beyond if cf_table);
 *                         mark != 0: the row is stamped pending for step t_done+1 (the backward of the forward this
 *                         launch precedes writes its gradient; a row that receives none holds zeros, and the real
 *                         step with g = 0 IS the zero-gradient step).  mark == 2: the same stamp, and the applied
 *                         rows are NOT cleared — the caller guarantees that the coming backward overwrites the gradient
 *                         row of every stamped row (and clears them itself, rp_zero_rows, if that backward never comes).
 *                         t_dev: device counter of completed steps.
 *   rp_lazy_adam_flush_deferred  the same for every row of the arena through t_target (g may be NULL when no
 *                         gradient arena exists yet); stamps last[row] = t_target.
 * Per row the same operations on the same values in the same order as rp_lazy_adam_rows: identical bits after a flush.
 * shadow_bf16 (both; NULL = none): the bf16 LOOKUP COPY of the tables ([rows, D] bf16, 16-byte aligned) of the bf16-storage
 * training mode — every parameter row the launch writes is also written there, rounded to nearest even; rp_rows_to_bf16
 * refreshes the run heads of a sorted key list after an update that went another way. */
int rp_lazy_adam_catchup(const int32_t *sorted_keys, int64_t n, int D, float *p, float *g, float *m, float *v,
                         int32_t *last, const float *step_scalars, int64_t t_done, int mark, double beta1, double beta2,
                         double eps, const float *cf_table, int64_t cf_from, const int32_t *t_dev, void *shadow_bf16,
                         rp_stream_t stream);
int rp_lazy_adam_flush_deferred(int64_t rows, int D, float *p, float *g, float *m, float *v, int32_t *last,
                                const float *step_scalars, int64_t t_target, double beta1, double beta2, double eps,
                                const float *cf_table, int64_t cf_from, void *shadow_bf16, rp_stream_t stream);
int rp_rows_to_bf16(const int32_t *sorted_keys, int64_t n, int D, const float *p, void *shadow_bf16, rp_stream_t stream);
int rp_lazy_adam_cf_table(const double *ns_d, int64_t t_end, int64_t cf_from, double beta1, double beta2, float *cf_table,
                          int64_t capacity, int64_t built_to, const int32_t *t_dev, rp_stream_t stream);

/* ---- request routing for row-sharded tables (rec_pangu_amd/sharded.py; no reference counterpart: the reference is
 * single-device).  Arena row r lives on rank r % world at local row r / world.
 *   rp_shard_keys   keys_out[f*B + b] = (owner << lbits) | local_row of id_f[b] (int32; range check / flag / row 0 as
 *                   the gather does); owner bits + lbits <= 31
 *   rp_route_build  from the SORTED keys (rp_sort_pairs_i32): slot_sorted [n] int32 = unique-request slot of the j-th
 *                   sorted request; slot_of_pair [n] int64 = slot of request p; uniq_rows [n] int64 whose first
 *                   counts[world] entries are the local rows to ask for, grouped by ascending owner (the all-to-all
 *                   send order); counts [world+1] int64 = unique requests per owner, then their total */
int rp_shard_keys(const int64_t *row_base, const int64_t *row_count, const int64_t *const *idx_ptrs, int F, int64_t B,
                  int world, int lbits, int32_t *keys_out, int32_t *err_flag, rp_stream_t stream);
int rp_route_workspace_bytes(int64_t n, int world, size_t *bytes);
int rp_route_build(void *workspace, size_t workspace_bytes, const int32_t *sorted_keys, const int32_t *sorted_pos,
                   int64_t n, int world, int lbits, int32_t *slot_sorted, int64_t *slot_of_pair, int64_t *uniq_rows,
                   int64_t *counts, rp_stream_t stream);
/* fixed-capacity form of the exchange (no host-side split sizes, hence no host sync per step): rewrites the compact
 * slots of rp_route_build as owner * capacity + index within the owner (slot_sorted in place, slot_of_pair) and fills
 * rows_padded[world * capacity] (zero-filled by the caller: unused slots ask for local row 0 and receive a zero
 * gradient).  More than `capacity` unique requests for one owner: bit 1 of *err_flag is set, the step is invalid. */
int rp_route_pad(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int world, int lbits,
                 int64_t capacity, const int64_t *counts, int32_t *slot_sorted, int64_t *slot_of_pair,
                 int64_t *rows_padded, int32_t *err_flag, rp_stream_t stream);
/* FIELD-MAJOR copy of a route's sorted request list (round 6).  Sorted by composite key the list is ordered (owner, field,
 * row); the first layer's backward launches (rp_embed_grad_seg / _ss / _smp) want field f's B requests at [f B, (f + 1) B)
 * with equal keys adjacent.  slot_fm / pos_fm [n] int32: the (slot, position) pairs of slot_sorted / sorted_pos moved
 * segment by segment — inside a field the order is (owner, row) = ascending slot, positions of a run keep their order.
 * n = F * B requests, world * F <= 1024 segments; delta: int64 scratch [world * F].  world == 1: the list is field-major
 * already (callers skip the call).  No reference counterpart (the reference is single-device: trainer.py:75). */
int rp_route_field_major(const int32_t *sorted_keys, const int32_t *sorted_pos, const int32_t *slot_sorted, int64_t n,
                         int64_t B, int world, int lbits, int32_t *slot_fm, int32_t *pos_fm, int64_t *delta,
                         rp_stream_t stream);

/* ---- LAUNCH PLANS: record a sequence of this library's kernel launches once, re-issue it with one call (csrc/plan.hip).
 * No reference counterpart (the reference's step loop is Python: model_pipeline.py:47-61); this is the host-side
 * mechanism behind rec_pangu_amd/graph_step.py's captured training step.  Between rp_plan_begin and rp_plan_end every
 * kernel launch any entry point of this library issues — from any host thread — is appended to the plan with its packed
 * arguments (and still issued: under a stream capture it becomes a graph node, otherwise it runs).  rp_plan_replay
 * re-issues the recorded launches with the recorded arguments on `stream`; launches recorded under rp_plan_section(1)
 * are independent of the others and go to a side stream owned by the plan, forked at rp_plan_fork_here (default: the start
 * of the replay) and joined at its end.  The caller guarantees that every address baked into the plan stays valid and that step numbers are read
 * on the device (t_dev arguments).  One plan may be recorded at a time, process-wide.
 *   rp_plan_info          launches recorded, those of section 1, distinct streams they were issued on while recording
 *   rp_graph_node_counts  kernel nodes / other nodes (memset, memcpy, ...) of a captured hipGraph_t: the check that a
 *                         captured step holds no launch the plan has not seen */
int rp_plan_begin(void **plan_out);
int rp_plan_section(int section);
int rp_plan_fork_here(void); /* the side section is forked in front of the NEXT main launch (default: start of the replay) */
/* rp_plan_section(2): an INLINE fork — the launches recorded under it run on a second side stream beside the main launches
 * recorded after them, from the point where they were recorded until rp_plan_join() (the first layer's weight gradient
 * beside the fused gather backward: both depend only on the masked dH).  The caller keeps every buffer those launches use
 * alive until the join: the capture's allocator assumes ONE stream and would hand a freed workspace to the next launch. */
int rp_plan_join(void);
/* explicit fork point of the inline section (2): its launches recorded after this mark depend on what the main stream held
 * HERE (main launches recorded between the mark and them run beside them), until the next rp_plan_join */
int rp_plan_fork2_mark(void);
/* Input rebinding: after rp_plan_end, name the addresses of the static input buffers the step was recorded on (n of them);
 * every 8-byte word of the recorded launch arguments that holds one is remembered (n_sites).  rp_plan_set_inputs(addrs[n])
 * then makes the next replays read buffer i from addrs[i] instead — the current batch's own tensors (same shape, dtype,
 * contiguity; alive until the replay has run), no staging copy. */
int rp_plan_bind_inputs(void *plan, const uint64_t *addrs, int n, int *n_sites);
int rp_plan_set_inputs(void *plan, const uint64_t *addrs, int n);
/* what rp_plan_bind_inputs would find, per input: sites[i] = argument words holding exactly addrs[i]; *n_interior = words that
 * point INSIDE buffer i (addrs[i] < word < addrs[i] + nbytes[i]): arguments derived from an input, which rp_plan_set_inputs
 * cannot re-point — the caller keeps its staging copy then (graph_step.py) */
int rp_plan_bind_report(void *plan, const uint64_t *addrs, const uint64_t *nbytes, int n, int32_t *sites, int *n_interior);
/* HOST MARKS: a step interleaved with work the library does not issue (the collectives of the row-sharded path) is recorded
 * as segments — rp_plan_host_mark() at each such point while recording (*index_out = 0, 1, ...; the foreign work is NOT
 * issued under the capture), rp_plan_replay_segment(plan, k, stream) for the launches between mark k - 1 and mark k, the
 * foreign work issued by the caller in between on the same stream (every launch of the segment on that one stream, in
 * recorded order, whatever section it was recorded under). */
int rp_plan_host_mark(int *index_out);
int rp_plan_replay_segment(void *plan, int seg, rp_stream_t stream);
/* the inline section (2) waits here for what the main stream holds at this point (a second dependency edge for a section
 * forked earlier; the fork mark while the section is not open yet) */
int rp_plan_side2_sync(void);
/* a non-blocking stream of the lowest priority the device offers (side streams that should yield to the main stream's
 * launches); the caller owns it */
int rp_stream_create_low(void **stream_out);
int rp_plan_is_recording(void);
int rp_plan_end(void *plan);
int rp_plan_info(void *plan, int *n_nodes, int *n_side, int *n_streams);
/* the streams sections 1 / 2 are re-issued on (NULL: the plan creates one); before the first replay */
int rp_plan_set_streams(void *plan, rp_stream_t side, rp_stream_t side2);
int rp_plan_inline_count(void *plan, int *n_inline);
int rp_plan_replay(void *plan, rp_stream_t stream);
/* Live timing of ONE launch inside replayed steps (bench.py's roofline: a replay runs no host code between its launches, so
 * nothing outside the library can bracket one of them).  rp_plan_set_probe(plan, k): the k-th recorded launch (0 ..
 * n_nodes - 1 of rp_plan_info, recorded order) of the following replays is bracketed by a HIP timing-event pair on the stream it
 * is issued on; -1 = off.  rp_plan_probe_ms: elapsed milliseconds of the last replay's pair (waits for it).
 * rp_plan_launch_name: the launch's (demangled) kernel name and section (0 main stream, 1 side, 2 inline side). */
int rp_plan_set_probe(void *plan, int launch);
int rp_plan_probe_ms(void *plan, float *ms);
/* Completion markers for the host's run-ahead bound (graph_step.py keeps at most 6 replayed steps in flight): an event
 * without timing and without the system-scope fence of a default event record (the host waits for it; it does not read
 * device memory on its strength).  (No counterpart in the reference.) */
int rp_marker_create(void **marker);
int rp_marker_record(void *marker, rp_stream_t stream);
int rp_marker_wait(void *marker);
int rp_marker_destroy(void *marker);
/* Host-side stall finder: the slowest single HIP call (kind 0 = kernel launch, 1 = event record, 2 = stream wait) issued by
 * the replays since the last reset, the plan node it belongs to (nodes, not launches: markers count) and its host time in
 * milliseconds.  reset != 0 starts a new window.  (No counterpart in the reference: its step is eager torch.) */
int rp_plan_slowest_call(void *plan, int *kind, int *node, double *ms, int reset);
int rp_plan_launch_name(void *plan, int launch, char *buf, int buf_len, int *section);
int rp_plan_destroy(void *plan);
int rp_graph_node_counts(void *graph, int *n_kernel, int *n_other);
/* dst_ptrs[i][0 : bytes[i]] = src_ptrs[i][..] for i < n in ONE launch (per 96 buffers): a batch of ~40 columns into the static
 * input buffers of a captured step.  Host arrays of device addresses; buffers must not overlap. */
int rp_multi_copy(void *const *dst_ptrs, const void *const *src_ptrs, const uint64_t *bytes, int n, rp_stream_t stream);

/* ---- sequence recall: the GRU recurrence of GRU4Rec and NARM (csrc/gru.hip) and NARM's attention readout (csrc/narm.hip) ----
 * replaces nn.GRU(batch_first=True) of rec_pangu/models/layers/sequence.py:231-251 (packed by length) and
 * rec_pangu/models/sequence/narm.py:21,49 (all L positions) with its autograd.  torch's gates in the order r, z, n, h_0 = 0;
 * ONE layer and direction per call, all L steps in one launch (plus one small launch that pads the weights).
 *   input: either ids int64 [B, L] + E [V, in] (rows gathered inside the kernel; an id outside [0, V) sets *err_flag and
 *          reads row 0) or a dense X [B, L, in]; exactly one of ids / X is non-NULL.
 *   W_ih [3H, in], W_hh [3H, H], b_ih / b_hh [3H] or both NULL.  steps int32 [B]: row b takes min(steps[b], L) steps
 *   (packed: its length; full: L).  last int32 [B]: h_last[b] = H_all[b, last[b]], zero when last[b] < 0 or >= steps[b].
 *   H_all [B, L, H]: zero at t >= steps[b]; it is all the backward keeps besides the inputs.
 * rp_gru_bwd: dH_all [B, L, H] and dh_last [B, H] are the arriving gradients (either may be NULL); dX [B, L, in] (NULL: not
 * wanted; in id mode it is the per-position gradient row rp_hist_rows_bwd reduces into dE); dW_ih, dW_hh (both or neither),
 * db_ih, db_hh (both or neither) are WRITTEN.  Deterministic: gate-gradient buffers [B, L, 3H] contracted by rp_linear_wgrad,
 * db_hh's n part through per-workgroup slabs added in workgroup order.
 * 1 <= in, H <= max_h of rp_gru_geometry (128) and L >= 1, RP_ERR_ARG otherwise (nothing is launched).  tb = batch rows per
 * workgroup.  Workspace (the same query for both calls, 16-byte aligned), A(x) = x rounded up to 256, Hp / Kp = H / in
 * rounded up to 32:
 *   A(12 Hp Kp) + A(12 Hp Hp) + 2 A(12 B L H) + A(4 H ceil(B / tb)) + (ids_mode ? A(4 B L in) : 0)
 *   + A(max(rp_linear_wgrad_workspace_bytes(B L, 3H, in), rp_linear_wgrad_workspace_bytes(B L, 3H, H))) */
int rp_gru_geometry(int *tb, int *max_h);
int rp_gru_workspace_bytes(int64_t B, int64_t L, int in, int H, int ids_mode, size_t *bytes);
int rp_gru_fwd(const int64_t *ids, const float *E, int64_t V, const float *X, int64_t B, int64_t L, int in, int H,
               const float *W_ih, const float *W_hh, const float *b_ih, const float *b_hh, const int32_t *steps,
               const int32_t *last, float *H_all, float *h_last, int32_t *err_flag, void *workspace, size_t workspace_bytes,
               rp_stream_t stream);
int rp_gru_bwd(const int64_t *ids, const float *E, int64_t V, const float *X, int64_t B, int64_t L, int in, int H,
               const float *W_ih, const float *W_hh, const float *b_ih, const float *b_hh, const int32_t *steps,
               const int32_t *last, const float *H_all, const float *dH_all, const float *dh_last, float *dX, float *dW_ih,
               float *dW_hh, float *db_ih, float *db_hh, void *workspace, size_t workspace_bytes, rp_stream_t stream);
/* dE[keys, :] += the sum of the per-position gradient rows g[pos, :] of every sorted (id, flat position) pair with that id,
 * id 0 skipped (padding_idx = 0): rp_hist_mean_bwd's walk over a [B L, D] gradient, one writer per row, a fixed order */
/* out[p, :] = E[ids[p], :] for p < n (the lookup alone, for a dropout between it and the GRU); an id outside [0, V) sets
 * *err_flag and reads row 0 */
int rp_hist_rows_fwd(const float *E, int64_t V, int D, const int64_t *ids, int64_t n, float *out, int32_t *err_flag,
                     rp_stream_t stream);
int rp_hist_rows_bwd(const int32_t *sorted_keys, const int32_t *sorted_pos, int64_t n, int D, int64_t V, const float *g,
                     int64_t ldg, float *dE, rp_stream_t stream);
/* NARM's readout: alpha[b, l] = sum_h v[h] (ids[b, l] > 0) sigmoid(q1[b, l, h] + q2[b, h]);
 *   out[b] = [sum_l alpha[b, l] G[b, l, :], ht[b, :]]  (out [B, 2H], alpha [B, L] kept for the backward).  1 <= H <= 128.
 * The backward WRITES dq1 [B, L, H], dq2 [B, H], dG [B, L, H], dht [B, H] and dv [H] (slabs of at most 1024 workgroups added in
 * workgroup order; workspace: rp_narm_attn_workspace_bytes = 4 H min(ceil(B / 4), 1024), at least 4 H). */
int rp_narm_attn_workspace_bytes(int64_t B, int H, size_t *bytes);
int rp_narm_attn_fwd(const float *q1, const float *q2, const float *v, const int64_t *ids, const float *G, const float *ht,
                     int64_t B, int64_t L, int H, float *alpha, float *out, rp_stream_t stream);
int rp_narm_attn_bwd(const float *q1, const float *q2, const float *v, const int64_t *ids, const float *G, const float *alpha,
                     const float *dout, int64_t B, int64_t L, int H, float *dq1, float *dq2, float *dG, float *dht, float *dv,
                     void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- sequence recall: the multi-interest encoder of MIND and ComirecDR (csrc/capsule.hip) ------------------------------------
 * replaces CapsuleNetwork of rec_pangu/models/layers/multi_interest.py:56-161 with its autograd and the readout loop of
 * rec_pangu/models/sequence/mind.py:44-49 / comirec.py:100-105.  Only rp_capsule_project_bwd_w takes a workspace.
 *
 * Projection (bilinear_type 2):  U[b, s, n] = sum_d W[s, n, d] X[b, s, d],  X [B, L, D], W [L, N, D] (N = K D), U [B, L, N];
 * one launch for all L positions on the exact-fp32 matrix core; the [B, L, N, D] product is never formed.
 *   rp_capsule_project_bwd_x WRITES dX[b, s, :] = dU[b, s, :] W[s];
 *   rp_capsule_project_bwd_w WRITES dW[s] = sum_b dU[b, s, :]^T X[b, s, :]: one workgroup per (position, 32 output rows, batch
 *   split) walks its rows front to back; with S > 1 splits a second launch adds the S partial sums in split order: a fixed
 *   order, no float atomics.  S = min(32, max(1, ceil(B / 512))) splits of R = 64 ceil(ceil(B / S) / 64) rows (so ceil(B / R)
 *   of them); workspace: rp_capsule_workspace_bytes(B, L, N, D) = 4 ceil(B / R) L N D bytes, 0 when one split covers the batch.
 * 1 <= D <= 128, 1 <= N <= 2048, 1 <= L <= 65535, RP_ERR_ARG otherwise (nothing is launched).
 *
 * Routing: per (b, k), Uk = U[b sb + k sk + l sl + d] (strides in floats; sk = 0: all K interests read the same [L, D] rows),
 * mask float [B, L] (non-zero = valid), b0 [B, K, L] initial logits or NULL for zeros, eps = 1e-9:
 *   for i = 0, 1, 2:  p = softmax_l(b_i) over ALL L positions;  c = p where mask != 0, else 0 (not renormalised);
 *                     s = c^T Uk;  n = |s|^2;  v = s n / (1 + n) / sqrt(n + eps);  if i < 2: b_{i+1} = b_i + Uk v
 *   out[b, k, :] = v of round 2.       A fully masked row gives exact zeros.
 * rp_capsule_route_bwd recomputes the rounds and WRITES dU with U's strides (sk = 0: the K contributions added in interest
 * order); stop_grad != 0: rounds 0 and 1 give U no gradient.  b0 takes no gradient.  Every result is bit-identical between runs.
 * Limits (rp_capsule_geometry): 1 <= K <= max_k (8), 1 <= L <= max_l (64), 1 <= D <= max_d (128) and
 * 4 max(K, 2) L (D + 1) <= lds_bytes (147456), RP_ERR_ARG otherwise (nothing is launched).  proj_tb / proj_tn: batch rows /
 * output columns per workgroup of the projection's forward.
 *
 * Readout: kidx[b] = argmax_k interests[b, k, :] . E[target[b], :] (the first maximum wins), best[b, :] = interests[b, kidx[b], :];
 * a target outside [0, V) sets *err_flag and reads row 0.  rp_interest_pick_bwd WRITES dout [B, K, D]: dbest[b] at kidx[b],
 * exact zeros elsewhere (no gradient through the scores). */
int rp_capsule_geometry(int *proj_tb, int *proj_tn, int *max_k, int *max_l, int *max_d, int *lds_bytes);
int rp_capsule_project_fwd(const float *X, const float *W, int64_t B, int64_t L, int N, int D, float *U, rp_stream_t stream);
int rp_capsule_project_bwd_x(const float *dU, const float *W, int64_t B, int64_t L, int N, int D, float *dX,
                             rp_stream_t stream);
int rp_capsule_workspace_bytes(int64_t B, int64_t L, int N, int D, size_t *bytes);
int rp_capsule_project_bwd_w(const float *dU, const float *X, int64_t B, int64_t L, int N, int D, float *dW, void *workspace,
                             size_t workspace_bytes, rp_stream_t stream);
int rp_capsule_route_fwd(const float *U, int64_t sb, int64_t sk, int64_t sl, const float *mask, const float *b0, int64_t B,
                         int K, int L, int D, float *out, rp_stream_t stream);
int rp_capsule_route_bwd(const float *U, int64_t sb, int64_t sk, int64_t sl, const float *mask, const float *b0,
                         const float *dout, int64_t B, int K, int L, int D, int stop_grad, float *dU, rp_stream_t stream);
int rp_interest_pick_fwd(const float *interests, const float *E, int64_t V, const int64_t *target, int64_t B, int K, int D,
                         float *best, int32_t *kidx, int32_t *err_flag, rp_stream_t stream);
int rp_interest_pick_bwd(const float *dbest, const int32_t *kidx, int64_t B, int K, int D, float *dout, rp_stream_t stream);

/* ---- sequence recall: SASRec's masked multi-head self-attention core (csrc/seq_attn.hip) --------------------------------------
 * replaces, with its autograd, what rec_pangu/models/layers/trainformer.py:70-92 does between the three projections and
 * `dense`.  Rows are already projected (biases added): q [., ldq] and kv [B L, ldkv] with K in columns [0, D) and V in
 * [D, 2 D), D = heads dh, head h at columns [h dh, (h + 1) dh) of each.  A stacked [B L, 3 D] buffer is q = qkv, kv = qkv + D,
 * ldq = ldkv = 3 D.  mask float [B, L], non-zero = content.  Per (b, head):
 *   ctx[i, :] = sum_j keep[i, j] / (1 - p) softmax_j(q_i . k_j / sqrt(dh) + m[i, j]) v_j,   m[i, j] = 0 where mask[b, j] != 0
 *   and j <= i, else -1e6f (added to the scaled fp32 score, as the reference adds its mask).  Keys j > i are skipped: a row
 *   with a visible key has the softmax over all L keys exactly; a row without one gets the softmax over its j <= i masked
 *   scores (finite; the reference's value there is quantised at the fp32 ulp of 1e6 and nothing should read it).
 * Full mode (qpos NULL, q_compact 0): q [B L, ldq], ctx [B L, D] head-interleaved, lse [B, heads, L] (max + log of the sum),
 *   the only thing kept for the backward; rp_seq_attn_bwd recomputes the probabilities from q, kv and lse, takes ctx and
 *   dctx [B L, D] and WRITES dq [B L, lddq] and dkv [B L, lddkv] (dK | dV); one launch each way, no [B, heads, L, L] tensor,
 *   no float atomics, bit-identical runs.
 * Last-row mode (qpos int64 [B]): ONE query per sample, position qpos[b] (clamped to L - 1); ctx [B, D], lse [B, heads];
 *   q_compact 0: the query is row b L + qpos[b] of q and the backward WRITES all L rows of the sample's dq (zeros but for
 *   that row); q_compact 1: q and dq are [B, .] buffers, row b.  dkv is written for all positions.  qpos[b] < 0: a zero ctx
 *   row, zero gradients, nothing of the sample is read.
 * Dropout: p in [0, 1); keep[i, j] is a pure function of (seed, offset, b, head, i, j) on dropout.hip's Philox4x32-10 stream
 *   (counter = ((b heads + head) L + i) * 32 + j / 4 and the offset, key = seed, draw j % 4, keep <=> draw >= p 2^32); one call
 *   takes one offset; the backward regenerates the decisions from the same (seed, offset).  p = 0 draws nothing.  The _dev
 *   forms read offset = *offset_dev + offset_delta on the device, as rp_dropout_fwd_dev.  rp_seq_attn_keep_mask WRITES the
 *   same decisions as uint8 [B, heads, L, L] through the same device function (offset_dev may be NULL): for tests.
 * Limits: 1 <= L <= 128, 1 <= dh <= 64, heads >= 1 (rp_seq_attn_fits: 1 inside, 0 outside; rp_seq_attn_geometry: max_l, max_dh,
 *   row_tile = query rows per wave, min_dh_tile = the smallest head-width tile: dh is rounded up to min_dh_tile 2^k);
 *   RP_ERR_ARG outside (nothing is launched).
 *
 * rp_seq_act_fwd / _bwd: the two feed-forward activations the GEMM epilogue lacks, elementwise over [M, N]:
 *   RP_SEQ_ACT_GELU x 0.5 (1 + erf(x / sqrt 2)), RP_SEQ_ACT_SWISH x sigmoid(x); the backward reads the saved INPUT x.
 * rp_seq_take_fwd: out[b, :] = x[b L + qpos[b], :D] (qpos clamped to L - 1; zeros for qpos[b] < 0), x [B L, ldx] -> [B, D];
 * rp_seq_take_bwd WRITES dx [B L, D]: dout[b] at that row, zeros elsewhere. */
#define RP_SEQ_ACT_GELU 0
#define RP_SEQ_ACT_SWISH 1
int rp_seq_attn_fits(int L, int heads, int dh);
int rp_seq_attn_geometry(int *max_l, int *max_dh, int *row_tile, int *min_dh_tile);
int rp_seq_attn_fwd(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                    const int64_t *qpos, int64_t B, int L, int heads, int dh, float p, uint64_t seed, uint64_t offset, float *ctx,
                    float *lse, rp_stream_t stream);
int rp_seq_attn_fwd_dev(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                        const int64_t *qpos, int64_t B, int L, int heads, int dh, float p, uint64_t seed, uint64_t offset_delta,
                        const uint64_t *offset_dev, float *ctx, float *lse, rp_stream_t stream);
int rp_seq_attn_bwd(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                    const int64_t *qpos, const float *ctx, const float *dctx, const float *lse, int64_t B, int L, int heads,
                    int dh, float p, uint64_t seed, uint64_t offset, float *dq, int64_t lddq, float *dkv, int64_t lddkv,
                    rp_stream_t stream);
int rp_seq_attn_bwd_dev(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                        const int64_t *qpos, const float *ctx, const float *dctx, const float *lse, int64_t B, int L, int heads,
                        int dh, float p, uint64_t seed, uint64_t offset_delta, const uint64_t *offset_dev, float *dq, int64_t lddq,
                        float *dkv, int64_t lddkv, rp_stream_t stream);
int rp_seq_attn_keep_mask(int64_t B, int L, int heads, float p, uint64_t seed, uint64_t offset, const uint64_t *offset_dev,
                          uint8_t *keep, rp_stream_t stream);
int rp_seq_act_fwd(const float *x, int64_t ldx, float *y, int64_t ldy, int64_t M, int N, int act, rp_stream_t stream);
int rp_seq_act_bwd(const float *dy, int64_t lddy, const float *x, int64_t ldx, float *dx, int64_t lddx, int64_t M, int N, int act,
                   rp_stream_t stream);
int rp_seq_take_fwd(const float *x, int64_t ldx, const int64_t *qpos, int64_t B, int L, int D, float *out, rp_stream_t stream);
int rp_seq_take_bwd(const float *dout, const int64_t *qpos, int64_t B, int L, int D, float *dx, rp_stream_t stream);

/* ---- sequence recall: NextItNet's residual blocks of dilated causal convolutions (csrc/causal_conv.hip) ------------------------
 * replaces ResBlockTwoMasked / ResBlockOneMasked of rec_pangu/models/layers/conv.py with their autograd: ONE block per call.
 *   two-masked (one_masked 0): out = relu(LN1(conv1_{2d}(relu(LN0(conv0_d(x)))))) + x, both convs C -> C with k taps;
 *   one-masked (one_masked 1): out = conv2(relu(LN2(conv1_d(relu(LN1(conv0(relu(LN0(x))))))))) + x, conv0 C -> C/2 and conv2
 *                              C/2 -> C are 1x1, conv1 C/2 -> C/2 has k taps.
 *   A conv's output position t reads input positions t - (k - 1 - j) dilation, j < k, zero where that is negative; weights
 *   [Cout, Cin, taps] and biases as nn.Conv1d keeps them.  LN: over the channels of one position, biased variance, eps 1e-5.
 * X [B, L, C]; lens int64 [B] (clamped to [0, L]): positions >= lens[b] are READ AS ZERO (the reference's masked_fill).
 * params / grads: HOST arrays of 12 device pointers — conv weight 0..2, conv bias 0..2, LN gamma 0..2, LN beta 0..2, in the
 *   order of the stages above (the third conv and LN are NULL for a two-masked block).
 * Full mode (last 0): out [B, L, C], every position; dout [B, L, C].
 * Last mode (last 1): out [B, C] = the block's output at position lens[b] - 1 (L - 1 when lens[b] = 0), computed from the
 *   R = 3 (k - 1) + 1 (two-masked) or k (one-masked) positions it depends on, anchor - i dilation; dout [B, C].
 * The forward keeps nothing but its output.  rp_causal_conv_bwd recomputes the stages from X and WRITES dX [B, L, C] (every
 *   element: zeros at positions >= lens[b] and, in last mode, at positions the read row does not depend on) and every
 *   gradient of `grads`: conv weights and biases by one rp_linear_wgrad per conv over buffers in the workspace, gamma / beta
 *   through per-workgroup slabs added in workgroup order.  No float atomics; bit-identical runs.
 * Launches, whatever B: forward 2; backward 7 (two-masked) or 9 (one-masked).
 * Limits (rp_causal_conv_fits: 1 inside, 0 outside; rp_causal_conv_geometry): 2 <= C <= max_c (128), 1 <= k <= max_k (5),
 *   1 <= L <= max_l (128), L C <= max_lc (8192), dilation >= 1; two tiles of the padded rows must fit lds_bytes.  Outside, a
 *   null pointer or a workspace that is too small: RP_ERR_ARG, nothing is launched.
 * Workspace (16-byte aligned), A(x) = x rounded up to 256, p(x) = x rounded up to 32, per conv c (Cin, Cout, taps):
 *   forward: sum_c 2 A(4 taps p(Cout) p(Cin));   backward: that + sum_c [A(4 B R Cout) if a LayerNorm follows conv c]
 *   + sum_c A(4 B R Cin taps) (B Cin for the one-masked conv2 in last mode) + A(4 ceil(B / TS) slab width)
 *   + A(max_c rp_linear_wgrad_workspace_bytes), R = L in full mode. */
int rp_causal_conv_fits(int L, int C, int k, int one_masked);
int rp_causal_conv_geometry(int *max_c, int *max_k, int *max_l, int *max_lc, int *lds_bytes);
int rp_causal_conv_workspace_bytes(int64_t B, int L, int C, int k, int one_masked, int last, int backward, size_t *bytes);
int rp_causal_conv_fwd(const float *X, const int64_t *lens, int64_t B, int L, int C, int k, int64_t dilation, int one_masked,
                       int last, const float *const *params, float *out, void *workspace, size_t workspace_bytes,
                       rp_stream_t stream);
int rp_causal_conv_bwd(const float *X, const int64_t *lens, const float *dout, int64_t B, int L, int C, int k, int64_t dilation,
                       int one_masked, int last, const float *const *params, float *dX, float *const *grads, void *workspace,
                       size_t workspace_bytes, rp_stream_t stream);

/* ---- sequence recall: session graphs and their gated graph cell (csrc/session_graph.hip) -------------------------------------
 * replaces generate_graph (rec_pangu/models/utils.py) and SRGNNConv / SRGNNCell (rec_pangu/models/layers/graph.py) with their
 * autograd, for SRGNN, NISER and GCSAN.  Sample b keeps its nodes in its own L slots: node v is row b L + v, [B, L, ...].
 *
 * rp_session_graph: hist int64 [B, L].  Per sample, over its items with id > 0 in order, s_0 .. s_{n-1}:
 *   nodes  int64 [B, L]  the distinct ids in ascending order (torch.unique's), 0 behind the node count;
 *   alias  int32 [B, L]  alias[l] = the node number of s_l for l < n, -1 behind (the items are compacted: a hole in hist does
 *                        not leave one here); transition l is alias[l] -> alias[l + 1];
 *   count  int32 [B]     the node count;
 *   indeg / outdeg int32 [B, L]  per node, counted over the multiset of the n - 1 transitions (0 behind the node count).
 *   1 <= L <= max_l (64, rp_session_graph_geometry; a wave per sample, samples_per_workgroup of them in a workgroup).
 *   One launch, integer work only.
 *
 * rp_ggnn_cell_fwd: ONE step of the cell over H [B, L, D] (rows behind the node count are read as zero) with the graph given
 *   by alias alone (lengths, node counts and degrees are counted from it; an entry outside [0, L) ends the sample's list):
 *     p_in = H W_in^T + b_in, p_out = H W_out^T + b_out,
 *     in[v] = sum over transitions u -> v of p_in[u] / outdeg(u), out[u] = sum over transitions u -> v of p_out[v] / indeg(v)
 *     (each sum in position order; zero without such a transition),
 *     gi = [in | out] W_ih^T + b_ih, gh = H W_hh^T + b_hh, r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n),
 *     h' = (1 - z) H + z n   on the rows of nodes, zero behind the node count.
 *   params / grads: HOST arrays of 8 device pointers: W_in [D, D], b_in [D], W_out [D, D], b_out [D], W_ih [3 D, 2 D],
 *   b_ih [3 D], W_hh [3 D, D], b_hh [3 D] (incomming_conv.lin, outcomming_conv.lin, lin_ih, lin_hh as nn.Linear keeps them).
 *   Outputs, each optional (NULL), at least one: Hout [B, L, D] = h'; seq_hidden [B, L, D], row l = h'[alias[l]] for l < n and
 *   zero behind; ht [B, D] = h'[alias[n - 1]], zero for n = 0.  Nothing is kept but the outputs.
 * rp_ggnn_cell_bwd: recomputes the step from H and WRITES dH [B, L, D] (zero behind the node count) and all 8 gradients.
 *   The arriving gradient of h' is dHout + the rows of dseq_hidden at the positions that name the node, in position order,
 *   + dht at the node of the last position; each of the three may be NULL.  Both reverse aggregations gather; dW and db of
 *   each Linear are one rp_linear_wgrad over rows stacked in the workspace.  No float atomics; bit-identical runs.
 * Launches, whatever B: forward 2 (padded weight copies + the cell); backward 2 + the four rp_linear_wgrad.
 * Limits (rp_ggnn_fits: 1 inside, 0 outside; rp_ggnn_geometry): 1 <= D <= max_d (128), 1 <= L <= max_l (64), B L < 2^29; a
 *   workgroup takes floor(rows_per_workgroup / L) samples; its tiles must fit lds_bytes.  Outside, a null pointer or a
 *   workspace that is too small: RP_ERR_ARG, nothing is launched.
 * Workspace (16-byte aligned), A(x) = x rounded up to 256, p = D rounded up to 32, s3 = 3 D rounded up to 4, k3 = s3 rounded
 *   up to 8: forward 2 A(4 p p) + A(24 p p) + A(12 p p); backward that + 2 A(4 p p) + A(8 p k3) + A(4 p k3) + A(8 B L D)
 *   + 2 A(4 B L s3) + 2 A(4 B L D) + A(the largest rp_linear_wgrad_workspace_bytes of the four).
 *
 * rp_l2norm_fwd / _bwd: y = x / max(|x|_2, 1e-12) per row of x [M, D] (F.normalize) and its gradient from x and dy; a row of
 *   zeros stays zero and passes a zero gradient; below 1e-12 the clamp is a constant (dx = dy / 1e-12). */
int rp_session_graph_geometry(int *max_l, int *samples_per_workgroup);
int rp_session_graph(const int64_t *hist, int64_t B, int L, int64_t *nodes, int32_t *alias, int32_t *count, int32_t *indeg,
                     int32_t *outdeg, rp_stream_t stream);
int rp_ggnn_geometry(int *max_d, int *max_l, int *rows_per_workgroup, int *lds_bytes);
int rp_ggnn_fits(int L, int D);
int rp_ggnn_cell_workspace_bytes(int64_t B, int L, int D, int backward, size_t *bytes);
int rp_ggnn_cell_fwd(const float *H, const int32_t *alias, int64_t B, int L, int D, const float *const *params, float *Hout,
                     float *seq_hidden, float *ht, void *workspace, size_t workspace_bytes, rp_stream_t stream);
int rp_ggnn_cell_bwd(const float *H, const int32_t *alias, const float *dHout, const float *dseq_hidden, const float *dht,
                     int64_t B, int L, int D, const float *const *params, float *dH, float *const *grads, void *workspace,
                     size_t workspace_bytes, rp_stream_t stream);
int rp_l2norm_fwd(const float *x, float *y, int64_t M, int D, rp_stream_t stream);
int rp_l2norm_bwd(const float *x, const float *dy, float *dx, int64_t M, int D, rp_stream_t stream);

/* ---- sequence recall: two-layer additive attention + pooling of the same rows (csrc/attn_pool.hip) ---------------------------
 * replaces STAMPLayer's attention (rec_pangu/models/layers/sequence.py:131-137) and MultiInterestSelfAttention.forward
 * (rec_pangu/models/layers/multi_interest.py:37-51) with their autograd.  X [B, L, D], valid [B, L] of 0 / 1, W1 [D, Dh],
 * W2 [Dh, K], c [B, Dh] or NULL:
 *     S[b, l, k] = sum_h W2[h, k] act((X[b, l, :] . W1)[h] + c[b, h])               act: RP_ACT_SIGMOID or RP_ACT_TANH
 *     norm RP_ATTN_POOL_MASK:    A = S valid; a sample without a valid position gives out = 0
 *     norm RP_ATTN_POOL_SOFTMAX: the score of a position with valid = 0 is the CONSTANT -1e9 (no gradient passes to S
 *                                there), then softmax over all L positions with max subtraction: a masked position has
 *                                weight exactly 0 unless the sample has no valid position, which pools uniformly
 *     out[b, k, :] = sum_l A[b, l, k] X[b, l, :]                     (rows at valid = 0 are read as they are)
 * rp_attn_pool_fwd writes out [B, K, D] and A [B, L, K]; A is all the backward needs besides the inputs: the hidden
 *   tensor [B, L, Dh] is never written.  rp_attn_pool_bwd recomputes it 32 columns at a time and WRITES dX [B, L, D],
 *   dW1 [D, Dh], dW2 [Dh, K] and, with c, dc [B, Dh] (dc and c: both or neither).  dW1 is one rp_linear_wgrad over the
 *   pre-activation gradients stacked in the workspace (transient, 4 B L Dhs bytes), dW2 goes through per-workgroup slabs
 *   added in workgroup order.  No float atomics; bit-identical runs.
 * Launches, whatever B: forward 2 (padded weight copy + the kernel); backward 3 + rp_linear_wgrad's.
 * Limits (rp_attn_pool_fits: 1 inside, 0 outside; rp_attn_pool_geometry): 1 <= D <= max_d (128), 1 <= Dh <= max_dh (512),
 *   1 <= K <= max_k (8), 1 <= L <= max_l (64), B L < 2^29; a workgroup takes floor(rows_per_workgroup / L) samples; its tiles
 *   must fit lds_bytes.  Outside, another act / norm, a null pointer or a workspace that is too small: RP_ERR_ARG, nothing
 *   is launched.
 * Workspace (16-byte aligned), A(x) = x rounded up to 256, p(x) = x rounded up to 32, Dhs = Dh rounded up to 4, Kb = Dhs
 *   rounded up to 8, n = ceil(B / floor(64 / L)) groups of samples walked by G = ceil(n / ceil(n / 1024)) workgroups:
 *   forward A(4 p(Dh) p(D)); backward that + A(4 p(D) Kb) + A(4 B L Dhs) + A(4 G Dh K)
 *   + A(rp_linear_wgrad_workspace_bytes(B L, D, Dh)). */
#define RP_ATTN_POOL_MASK 0
#define RP_ATTN_POOL_SOFTMAX 1
int rp_attn_pool_geometry(int *max_d, int *max_dh, int *max_k, int *max_l, int *rows_per_workgroup, int *lds_bytes);
int rp_attn_pool_fits(int L, int D, int Dh, int K);
int rp_attn_pool_workspace_bytes(int64_t B, int L, int D, int Dh, int K, int backward, size_t *bytes);
int rp_attn_pool_fwd(const float *X, const float *valid, const float *W1, const float *W2, const float *c, int64_t B, int L,
                     int D, int Dh, int K, int act, int norm, float *out, float *A, void *workspace, size_t workspace_bytes,
                     rp_stream_t stream);
int rp_attn_pool_bwd(const float *X, const float *valid, const float *W1, const float *W2, const float *c, const float *A,
                     const float *dout, int64_t B, int L, int D, int Dh, int K, int act, int norm, float *dX, float *dW1,
                     float *dW2, float *dc, void *workspace, size_t workspace_bytes, rp_stream_t stream);

/* ---- sequence recall: the key-padding (non-causal) mode of the sequence attention core (csrc/seq_attn_keypad.hip) ----------------
 * the attention of the reference's BERT4RecEncoder (rec_pangu/models/layers/sequence.py:150-186).  Layouts, modes (full,
 * last-row with qpos, q_compact) and limits are rp_seq_attn_fwd's; the differences: every query row attends to every CONTENT
 * key (mask[b, j] != 0), whatever its position; a masked key is skipped (probability exactly 0, so its dK and dV rows are
 * exactly 0) instead of taking an additive score; a sample without a content key gets zero ctx rows, lse 0 and zero
 * gradients; there is no dropout; the backward takes no ctx (its delta comes from the recomputed probabilities).  One launch each way, nothing of size L x L stored, no float atomics, bit-identical runs.
 * Outside rp_seq_attn_fits: RP_ERR_ARG, nothing is launched. */
int rp_seq_attn_keypad_fwd(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                           const int64_t *qpos, int64_t B, int L, int heads, int dh, float *ctx, float *lse, rp_stream_t stream);
int rp_seq_attn_keypad_bwd(const float *q, int64_t ldq, int q_compact, const float *kv, int64_t ldkv, const float *mask,
                           const int64_t *qpos, const float *dctx, const float *lse, int64_t B, int L, int heads, int dh, float *dq,
                           int64_t lddq, float *dkv, int64_t lddkv, rp_stream_t stream);

/* ---- sequence recall: the in-batch contrastive loss of CLRec and ContraRec (csrc/contrast.hip) -----------------------------------
 * replaces, with its autograd, rec_pangu/models/sequence/clrec.py:65-102 and contrarec.py:93-144, which materialise the
 * [n, m] similarity matrix about seven times.  a [n, lda], b [m, ldb] fp32 rows of D columns, la [n], lb [m] int64 labels,
 * l_ij = (a_i . b_j) / temperature.  b NULL: the symmetric form (b = a, lb = la, m = n; pass lb NULL or la), the only one
 * that takes exclude_self.  Per row i, N_i = all j (exclude_self: j != i), P_i = { j in N_i : la[i] == lb[j] }, c_i = |P_i|:
 *   m_i = max_j l_ij over ALL j,  lse_i = m_i + log(sum_{j in N_i} exp(l_ij - m_i) + 1e-10),
 *   loss = (scale / n) sum_i -(sum_{j in P_i} (l_ij - lse_i)) / (c_i + 1e-10)          (a row with c_i = 0 adds 0).
 * rp_contrast_fwd writes loss [1], lse [n] (DOUBLE: a float at |lse| ~ 24 would round away log(sum) of a row whose positive
 * holds nearly all of its probability) and c [n] (the counts as floats): all the backward needs besides the inputs.
 * rp_contrast_bwd recomputes p_ij = exp(l_ij - lse_i) tile by tile and WRITES, with g = gloss[0] (device) and
 *   q_ij = [j in N_i] p_ij c_i / (c_i + 1e-10) - [j in P_i] / (c_i + 1e-10):
 *   da [n, ldda] = g scale / (n T) sum_j q_ij b_j,  db [m, lddb] = g scale / (n T) sum_i q_ij a_i   (either may be NULL);
 *   symmetric form: the one result da + db in da (db must be NULL).
 * No [n, m] tensor in either direction; every sum in a fixed order, no float atomics, bit-identical runs.  Products follow
 * rp_matmul_products (fp32-faithful by default), as rp_softmax_ce_fwd.
 * Limits: n, m >= 1, 1 <= D <= max_d (rp_contrast_geometry: ta / tb = rows of a / b per tile, max_d = 128, max_splits of m;
 *   rp_contrast_fits: 1 inside, 0 outside), temperature > 0; outside, a null pointer or a workspace too small: RP_ERR_ARG,
 *   nothing is launched.  Workspace: rp_contrast_workspace_bytes(n, m, D) bytes (pass the asymmetric m, or n for the
 *   symmetric form), 16-byte aligned, one size for both directions. */
int rp_contrast_fits(int D);
int rp_contrast_geometry(int *ta, int *tb, int *max_d, int *max_splits);
int rp_contrast_workspace_bytes(int64_t n, int64_t m, int D, size_t *bytes);
int rp_contrast_fwd(const float *a, int64_t lda, const float *b, int64_t ldb, const int64_t *la, const int64_t *lb, int64_t n,
                    int64_t m, int D, float temperature, int exclude_self, float scale, double *lse, float *c, float *loss,
                    void *workspace, size_t workspace_bytes, rp_stream_t stream);
int rp_contrast_bwd(const float *a, int64_t lda, const float *b, int64_t ldb, const int64_t *la, const int64_t *lb,
                    const double *lse, const float *c, const float *gloss, int64_t n, int64_t m, int D, float temperature,
                    int exclude_self, float scale, float *da, int64_t ldda, float *db, int64_t lddb, void *workspace,
                    size_t workspace_bytes, rp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* REC_PANGU_HIP_H */
