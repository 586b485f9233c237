/*
 * clipk.h — C ABI of libclipk.so: the MI355X (gfx950 / CDNA4) kernels behind the CLIP-style
 * dual-encoder contrastive path of SrikarK-code/clip-dplm.
 *
 * The reference has NO FFI / operator boundary of its own: its boundary is the Python
 * nn.Module API of old/clip.py.  Each entry point below therefore cites the ATen call site(s) in the
 * reference that it replaces; the Python mirror of the module API lives in clip_dplm_amd/ and binds these
 * symbols through ctypes (clip_dplm_amd/_ffi.py).  INTEGRATION.md shows the reference-side stub.
 *
 * Conventions (every entry point):
 *   - extern "C", plain device pointers + sizes, no torch types;
 *   - returns CLIPK_OK (0) or a negative clipk_status; never throws, never allocates, never syncs;
 *   - enqueues on the caller's hipStream_t (passed as void*), so ordering is the caller's stream order;
 *   - every buffer (outputs, workspaces) is owned by the caller; workspace sizes come from
 *     clipk_*_workspace() helpers; stateless and re-entrant;
 *   - bf16 tensors are raw uint16 storage ("bf16"), f32 are float; row-major with explicit leading
 *     dimensions in ELEMENTS.
 */
#ifndef CLIPK_H
#define CLIPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum clipk_status {
  CLIPK_OK = 0,
  CLIPK_ERR_BAD_ARG = -1,       /* null pointer / non-positive dim / misaligned pointer            */
  CLIPK_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels tile (see each entry point)       */
  CLIPK_ERR_LAUNCH = -3         /* hipGetLastError() != hipSuccess after the launch                 */
} clipk_status;

typedef enum clipk_dtype { CLIPK_BF16 = 0, CLIPK_F32 = 1, CLIPK_U8 = 2 } clipk_dtype;
typedef enum clipk_act { CLIPK_ACT_NONE = 0, CLIPK_ACT_RELU = 1, CLIPK_ACT_GELU = 2, CLIPK_ACT_CELU = 3,
                         CLIPK_ACT_SOFTPLUS = 4 } clipk_act;

int clipk_version(void);          /* ABI version, bumped on any signature change */
const char* clipk_arch(void);     /* "gfx950" */
const char* clipk_status_string(int status);

/* Kernel-selection options (process-wide, explicit; the library never reads environment variables).  Every value
 * of every option computes the same results: they pick between kernels / schedules that tests and tools/ compare.
 * Names: gemm_kernel (-1 auto, 1 generic, 2 128x128, 3 persistent 256x256, 4 persistent 128x256 with two workgroups per CU), gemm_epi_generic, gemm_bm, gemm_stages,
 * gemm_nwg, gemm_stagger, epi_nt, wgrad_kernel (-1 auto, 2, 3), attn_whole_fwd, attn_fused_bwd (-1 auto, 0, 1),
 * attn_fused_waves (0 auto: 4 waves for head dims <= 32, 8 for 96; 4; 8), attn_row_stores (0, 2: forward write-back of rotated rows from LDS), gemm_f32_splits (0 auto, 1 .. 8: cross-workgroup splits of the skinny f32 Linear), simce_kernel (-1 auto, 1 first-generation, 2 tiled LSE pass), retrieval_splits (0 auto, n > 0: key-range splits of clipk_sim_topk / clipk_sim_rank).  Unknown name -> CLIPK_ERR_BAD_ARG.  (The reference has no counterpart: its kernels are
 * ATen's.) */
int clipk_set_option(const char* name, int value);
int clipk_get_option(const char* name, int* value);
int clipk_reset_options(void);

/* ------------------------------------------------------------------------------------------------
 * Linear (GEMM + fused epilogue), bf16 MFMA, f32 accumulate.
 *   C[M,N] = epilogue( A[M,K] · B[N,K]^T )
 *   epilogue(v) : v += bias[n];  if out_preact: out_preact = v (bf16);  v = act(v);
 *                 if dact_aux: v *= act'(dact_aux[m,n]);  if residual: v += residual[m,n];  C = v
 * Replaces nn.Linear (+ReLU/GELU, + residual add) at old/clip.py:11,16,27,29,31; the QKV / out-proj /
 * FFN Linear layers of nn.TransformerEncoderLayer (current/rna_clip_codes.ipynb:1915) and of the
 * third-party EsmLayer (transformers modeling_esm.py:362-374,517-521) called at
 * triple_flow/3_esm_integration.py:118-119.  With B = W^T (a [K_out,N_in] copy) it is the input
 * gradient dX = dY·W of the same layers.
 * Requirements: K % 8 == 0, N % 8 == 0, lda/ldb/ldc/... % 8 == 0, pointers 16-byte aligned.
 */
typedef struct clipk_gemm_args {
  const void* A; int64_t lda;          /* bf16 [M,K]                                       */
  const void* B; int64_t ldb;          /* bf16 [N,K]  (nn.Linear weight layout)            */
  void* C; int64_t ldc; int c_dtype;   /* bf16 or f32 [M,N]                                */
  int M, N, K;
  const float* bias;                   /* f32 [N] or NULL                                  */
  int act;                             /* clipk_act applied after bias                     */
  void* out_preact; int64_t ldp;       /* optional bf16 [M,N]: value before activation     */
  const void* dact_aux; int64_t ldd;   /* optional bf16 [M,N]: multiply by act'(aux)       */
  int dact;                            /* clipk_act whose derivative is applied to aux     */
  const void* residual; int64_t ldr; int r_dtype; /* optional [M,N] bf16/f32, added last   */
  float alpha;                         /* scale applied to the raw product before bias     */
  /* dropout on the value after the activation (and before act'(aux) / the residual add): v *= keep / (1 - p), with
   * keep = hash(drop_seed, m * N + n) >= drop_p * 2^32 — nn.Dropout after out_proj / linear2 / the FFN activation of
   * nn.TransformerEncoderLayer(dropout = p) (current/rna_clip_codes.ipynb:1915).  The same (seed, p) on the matching
   * backward GEMM reproduces the mask; nothing is stored.  drop_p = 0: off. */
  float drop_p; uint32_t drop_seed;
  /* rotary position embedding on the first rope_cols output columns (ESM-2's fused [q | k | v] projection: the q and k
   * thirds), applied to the f32 value (product + bias) before the single bf16 rounding: heads are rope_hd consecutive
   * columns, out[d] = x[d] cos[pos, d mod hd/2] -/+ x[d +/- hd/2] sin[pos, d mod hd/2] (rotate-half, transformers
   * modeling_esm.py:48-52,74-79), pos = (row + rope_row0) mod rope_L, tables f32 [rope_L, rope_hd/2].  Replaces the
   * separate clipk_rope_qk pass after the projection (one read + one write of q and k per layer).  rope_cos = NULL:
   * off.  Requirements: bf16 output, no activation / residual / aux / dropout, rope_hd in {16, 32, 64},
   * rope_cols % rope_hd == 0, K % 32 == 0; anything else returns CLIPK_ERR_UNSUPPORTED (never silently unrotated). */
  const float* rope_cos; const float* rope_sin; int rope_L, rope_hd, rope_cols, rope_row0;
  /* aux_dtype = CLIPK_U8 (act / dact must be GELU): the auxiliary tensor of the FFN pair is the DERIVATIVE GELU'(v) as an
   * 8-bit code instead of the bf16 pre-activation v - out_preact receives u8 [M, N] codes (ldp in bytes, % 8 == 0),
   * dact_aux is read as such codes and the product is multiplied by the decoded value: code = round(GELU'(v) * 200 + 26),
   * decoded as -0.13 + 0.005 code: 256 levels from -0.13 to 1.145 (GELU' lies in [-0.129, 1.129]) with GELU' = 0 and
   * GELU' = 1 - what dead and saturated units take - code points themselves, error <= 0.0025 - half the bytes of the
   * pre-activation in the two store-bound FFN epilogues of EsmLayer / nn.TransformerEncoderLayer(activation = gelu)
   * (modeling_esm.py:517-521; run1/configuration_hybrid_clip.py:75 hidden_act), nothing but the backward's GELU' factor
   * is affected.  CLIPK_BF16 (0): the pre-activation itself, as before. */
  int aux_dtype;
  /* rope_interleaved != 0 (with rope_cos / rope_sin / rope_L / rope_hd / rope_cols): the heads of the first rope_cols output
   * columns are in PAIR-INTERLEAVED order - columns 2 j and 2 j + 1 of a head hold what rotate-half calls x[j] and
   * x[j + hd/2] (the B operand's rows were permuted accordingly: clipk_cast_transpose il_hd / il_rows) - and are rotated as
   * neighbours: out[2j] = x1 cos[pos, j] - x2 sin[pos, j], out[2j+1] = x2 cos[pos, j] + x1 sin[pos, j].  Any rope_hd % 8 == 0
   * (ESM-2-35M's 24, which does not tile the kernels' 64-column slices).  q . k does not depend on a common order of the head
   * dim, so attention runs on such q / k as it is (clipk_attn_fwd without tables; clipk_attn_bwd with prerotated = 2). */
  int rope_interleaved;
} clipk_gemm_args;
int clipk_gemm_nt(const clipk_gemm_args* args, void* stream);

/* Weight gradient: dW[N,K] (+)= dY[M,N]^T · X[M,K]   (contraction over the M tokens), f32 output.
 * Replaces autograd's mm(dY^T, X) for every nn.Linear above.  Split over M with per-split f32 slabs in
 * `workspace` followed by a deterministic reduce (no float atomics).  Also emits db[N] = colsum(dY)
 * when dbias != NULL.  accumulate != 0 adds into dW/dbias instead of overwriting.
 * Requirements: N % 8 == 0, K % 8 == 0. */
size_t clipk_gemm_wgrad_workspace(int M, int N, int K);
/* il_rows > 0: dY's first il_rows columns are in pair-interleaved head order (heads of il_hd columns: clipk_gemm_nt
 * rope_interleaved, clipk_attn_bwd prerotated = 2); their gradient rows are written to the rows of dW / entries of dbias of
 * the ORIGINAL order, so the master weights and their gradients never see the permutation. */
int clipk_gemm_wgrad(const void* dY, int64_t lddy, const void* X, int64_t ldx,
                     float* dW, int64_t lddw, float* dbias,
                     int M, int N, int K, int accumulate, int il_hd, int il_rows,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused similarity + cross-entropy ("simce"), exact-f32 MFMA (v_mfma_f32_32x32x2_f32), never
 * materialises the logits.
 *   S[i,j] = scale * <X[i,:], Y[j,:]>,  label(i) = label_offset + i
 *   lse[i] = log sum_j exp(S[i,j])  over the Ny keys of Y plus the Nc keys of Yc (cache negatives)
 *   pos[i] = S[i, label(i)]
 * Replaces matmul(a, b.t()) * logit_scale + cross_entropy at old/clip.py:66-67 + old/ablation.py:16,
 * current/rna_clip_codes.ipynb:1950-1953 (both directions: call twice with X/Y swapped) and
 * old/clip_opt.py:115-121,130-151 (cache columns).  Rows of X are this rank's samples, Y holds the
 * all-gathered batch (old/clip_opt.py:102-112).
 * Requirements: P % 4 == 0, P <= 768.  workspace: clipk_simce_workspace(Mx, Ny + Nc, P) bytes (covers both
 * clipk_simce_lse and clipk_simce_grad). */
size_t clipk_simce_workspace(int Mx, int Nkeys, int P);
int clipk_simce_lse(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc,
                    int P, const float* scale /* device scalar = exp(logit_scale), clamped by caller */,
                    int label_offset, float* lse /*[Mx]*/, float* pos /*[Mx]*/,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Gradient of  L = (w_row * sum_i (lse_row[i] - pos[i]) + w_col * sum_j (lse_col[j] - pos[j])) / Bg
 * with respect to X rows (this rank's rows of one modality):
 *   G[i,j] = ( w_row * exp(S[i,j]-lse_x[i]) + w_col * exp(S[i,j]-lse_y[j]) - (w_row+w_col)*[j==label(i)] ) / Bg
 *   dX[i,:] = scale * sum_j G[i,j] * Y[j,:]  (+ cache keys: only the w_row term, no positives)
 *   dscale_partial[i] = sum_j G[i,j] * <X[i],Y[j]>       (d/d scale; caller multiplies by scale for
 *                                                        d/d logit_scale and halves the double count)
 * lse_x: [Mx] LSE of the rows of X over all keys;  lse_y: [Ny] LSE of each key over all queries
 * (the other direction), all-gathered across ranks by the caller. */
int clipk_simce_grad(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc,
                     int P, const float* scale, int label_offset,
                     const float* lse_x, const float* lse_y, float w_row, float w_col, float inv_bg,
                     float* dX /*[Mx,P]*/, float* dscale_partial /*[Mx]*/,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The same with the loss' incoming gradient folded in: `upstream` (device scalar, or NULL = 1) multiplies inv_bg inside the
 * kernel - autograd's `grad_output * dX` after the fact was three more launches on [B, P] / [1] tensors per step
 * (loss.backward() hands 1.0; upstream = 1 gives clipk_simce_grad's bits). */
int clipk_simce_grad_scaled(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc,
                            int P, const float* scale, int label_offset,
                            const float* lse_x, const float* lse_y, float w_row, float w_col, float inv_bg,
                            const float* upstream, float* dX /*[Mx,P]*/, float* dscale_partial /*[Mx]*/,
                            void* workspace, size_t workspace_bytes, void* stream);
/* loss[0] = (w_row * sum_i (lse_r[i] - pos_r[i]) + w_col * sum_i (lse_c[i] - pos_c[i])) / bg from the two clipk_simce_lse
 * results in one launch, fixed summation order (the two F.cross_entropy means and their average of
 * rna_clip_codes.ipynb:1952-1953; old/ablation.py:16 with w_col = 0 and lse_c = pos_c = NULL). */
int clipk_ce_combine(const float* lse_r, const float* pos_r, const float* lse_c, const float* pos_c, int n,
                     float w_row, float w_col, float bg, float* loss, void* stream);

/* Class-aware InfoNCE: pairs carry class ids, so pairs that share a partner (one RBP bound by many RNAs, one
 * perturbation over many cells) are no longer each other's negatives.  For query row i with diagonal key
 * l = label_offset + i, keys j over the Ny batch keys and then the Nc cache keys, S[i,j] = scale * <X_i, Y_j>:
 *   same[i,j] = (j < Ny) and (j == l or cls_y[j] == cls_x[i])       the diagonal always; cache keys never
 *   D_i       = all keys except {j != l : same[i,j]}   (same_class = CLIPK_SAME_CLASS_MASK)
 *             = all keys                               (same_class = CLIPK_SAME_CLASS_POSITIVE, supervised contrastive)
 *   N_i = |D_i|,  c_i = #{j : same[i,j]}
 *   q[i,j]    = [j == l] (mask)  or  same[i,j] / c_i (positive)
 *   T[i,j]    = (1 - eps) q[i,j] + eps / N_i [j in D_i]        eps = label smoothing in [0, 1)
 *   lse[i] = log sum_{j in D_i} exp S[i,j],   tgt[i] = sum_j T[i,j] S[i,j],   cnt[i] = c_i
 * The loss is clipk_ce_combine with tgt in place of pos.  With no ids (cls_x = cls_y = NULL: all distinct) and eps > 0
 * this is F.cross_entropy(S, arange, label_smoothing=eps) over [S | S_cache] (torch's convention: eps / N on every key,
 * the diagonal's included); with distinct ids and eps = 0 it is the plain loss.  Its lse then has the bits of
 * clipk_simce_lse's tiled LSE pass, which clipk_simce_lse runs for Mx >= 64 and Ny + Nc >= 64 (or with option
 * simce_kernel = 2); for smaller shapes clipk_simce_lse defaults to the first-generation kernel, whose summation order
 * differs, and the two agree to rounding only.
 * cls_x [Mx], cls_y [Ny]: device int64, both or neither.  label_offset + Mx <= Ny.  All work stays on the device.
 * Requirements: P % 4 == 0, P <= 512 (else CLIPK_ERR_UNSUPPORTED).  workspace: clipk_simce_cls_workspace(Mx, Ny + Nc, P)
 * bytes (covers both passes).  Key-split partials merge in a fixed order: deterministic. */
enum { CLIPK_SAME_CLASS_MASK = 0, CLIPK_SAME_CLASS_POSITIVE = 1 };
size_t clipk_simce_cls_workspace(int Mx, int Nkeys, int P);
int clipk_simce_lse_cls(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                        const float* scale, int label_offset, const int64_t* cls_x, const int64_t* cls_y,
                        int same_class, float eps, float* lse /*[Mx]*/, float* tgt /*[Mx]*/, float* cnt /*[Mx]*/,
                        void* workspace, size_t workspace_bytes, void* stream);
/* Gradient of (w_row * sum_i (lse_x[i] - tgt_x[i]) + w_col * sum_j (lse_y[j] - tgt_y[j])) * inv_bg (* upstream) w.r.t.
 * the rows of X, the column direction being the keys' own CE over the pair rows (its sets, counts and targets primed):
 *   G[i,j] = w_row ([j in D_i] exp(S[i,j] - lse_x[i]) - T[i,j]) + w_col ([i in D'_j] exp(S[i,j] - lse_y[j]) - T'[j,i])
 * same is symmetric, so i in D'_j iff j in D_i;  T'[j,i] uses c'_j = cnt_y[j] and N'_j from nkeys_y, the column
 * direction's key count (Ny, plus the cache rows when the direction that owns them is the column one).  dX and
 * dscale_partial follow from G as in clipk_simce_grad.  cnt_x / cnt_y: the cnt outputs of clipk_simce_lse_cls for
 * each direction (cnt_x may be NULL when w_row == 0, cnt_y when w_col == 0). */
int clipk_simce_grad_cls(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                         const float* scale, int label_offset, const float* lse_x, const float* lse_y,
                         const float* cnt_x, const float* cnt_y, const int64_t* cls_x, const int64_t* cls_y,
                         int same_class, float eps, int nkeys_y, float w_row, float w_col, float inv_bg,
                         const float* upstream, float* dX /*[Mx,P]*/, float* dscale_partial /*[Mx]*/,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Hard-negative-weighted InfoNCE: the 'hard_negative' loss variant of run1/full.py:347, switched on by
 * use_hard_negatives / hard_negative_weight (run1/configuration_hybrid_clip.py:105-106; tong/configs/default.yaml:55).
 * The reference names the variant and its weight only; the arithmetic is the importance weighting of Robinson, Chuang,
 * Sra and Jegelka, "Contrastive Learning with Hard Negative Samples" (ICLR 2021) with tau_plus = 0, beta their
 * concentration parameter.  For query row i, diagonal key l = label_offset + i, S[i,j] = scale * <X_i, Y_j> over the Ny
 * batch keys and then the Nc cache keys:
 *   Neg_i   = { j != l } minus, with class ids, { j < Ny : cls_y[j] == cls_x[i] }   (the "mask" rule; cache keys stay)
 *   n_i     = |Neg_i|
 *   A_i     = log sum_{Neg_i} exp(beta S[i,j]),   C_i = log sum_{Neg_i} exp((1 + beta) S[i,j])
 *   logNg_i = log n_i + C_i - A_i      = log sum_{Neg_i} w_ij exp S[i,j],  w_ij = exp(beta S_ij) / mean_{Neg_i} exp(beta S_ik)
 *   lse_h[i] = logaddexp(S[i,l], logNg_i),   pos[i] = S[i,l],   loss_i = lse_h[i] - pos[i]
 *   n_i = 0: logNg_i = -inf, loss_i = 0, zero gradient.
 * beta = 0 is the plain loss; for beta >= 0, loss_i >= the plain loss_i.  The batch loss is clipk_ce_combine.
 * coef [3][Mx]: what the gradient pass needs of a row, q = exp(logNg - lse_h), k1 = log(q (1 + beta)) - C,
 * k2 = log(q beta) - A (-inf where the factor is 0).
 * beta >= 0 and finite (else CLIPK_ERR_BAD_ARG); cls_x [Mx], cls_y [Ny]: device int64, both or neither;
 * label_offset + Mx <= Ny; P % 4 == 0, P <= 512 (else CLIPK_ERR_UNSUPPORTED).  workspace:
 * clipk_simce_hard_workspace(Mx, Ny + Nc, P) bytes (covers both passes).  Exact-f32 MFMA on the tiling of
 * clipk_simce_lse; no atomics, no allocation, no synchronisation; key-split partials merge in a fixed order. */
size_t clipk_simce_hard_workspace(int Mx, int Nkeys, int P);
int clipk_simce_lse_hard(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                         const float* scale, float beta, int label_offset, const int64_t* cls_x, const int64_t* cls_y,
                         float* lse_h /*[Mx]*/, float* pos /*[Mx]*/, float* coef /*[3][Mx]*/, void* workspace,
                         size_t workspace_bytes, void* stream);
/* Gradient of (w_row * sum_i loss_i + w_col * sum_j loss'_j) * inv_bg (* upstream) w.r.t. the rows of X, the column
 * direction being every key's own loss over the pair rows (no cache there).  Per direction, on its negatives,
 *   g[i,j] = q_i [(1 + beta) exp((1 + beta) S_ij - C_i) - beta exp(beta S_ij - A_i)]
 *          = exp((1 + beta) S_ij + k1_i) - exp(beta S_ij + k2_i),     g[i,l] = -q_i,  g = 0 on masked keys
 *   G[i,j] = (w_row g_row[i,j] + w_col g_col[j,i]) * inv_bg (* upstream)
 * and dX, dscale_partial follow from G as in clipk_simce_grad.  coef_x [3][Mx]: the rows' coefficients; coef_y [3][Ny]:
 * those of every batch key's own direction (with w_col == 0: q = 0, k1 = k2 = -inf). */
int clipk_simce_grad_hard(const float* X, int Mx, const float* Y, int Ny, const float* Yc, int Nc, int P,
                          const float* scale, float beta, int label_offset, const float* coef_x, const float* coef_y,
                          const int64_t* cls_x, const int64_t* cls_y, float w_row, float w_col, float inv_bg,
                          const float* upstream, float* dX /*[Mx,P]*/, float* dscale_partial /*[Mx]*/,
                          void* workspace, size_t workspace_bytes, void* stream);

/* Batched form for several same-shape contrastive problems on one logit scale — the tri-modal ContrastiveModel of
 * current/tf_clip_codes (1).ipynb:13150-13163 (cell x pert, cell x protein, pert x protein, each symmetric) is six
 * directed problems (X = E[pairs[2i]], Y = E[pairs[2i+1]]), computed by ONE launch per pass (grid z = problem):
 *   lse_pairs : lse[i][b] = LSE_j scale <X_b, Y_j>, pos[i][b] = scale <X_b, Y_b>
 *   grad_pairs: dX[i] = complete gradient of (w_row CE_rows + w_col CE_cols)(X, Y) * inv_bg w.r.t. the rows of X,
 *               using lse[i] for the rows and lse[reverse[i]] (the problem with X and Y exchanged) for the keys.
 * E: f32 [nmod][B][P] contiguous; pairs / reverse: HOST int arrays; npairs <= 6.
 * grad_pairs needs a P slice per wave (P over 1, 2, 4 or 8 waves of at most 128 columns, rounded up to 8) that is a
 * multiple of 32, as P = 32, 64, 96, 128, 192, 256, 384, 512, 768 give: CLIPK_ERR_UNSUPPORTED otherwise
 * (clipk_simce_grad_pairs_cls without ids, with cnt = 1, is the same gradient at every P % 4 == 0, P <= 512). */
size_t clipk_simce_pairs_workspace(int npairs, int B, int P);
int clipk_simce_lse_pairs(const float* E, int nmod, int B, int P, const int* pairs, int npairs, const float* scale,
                          float* lse /*[npairs][B]*/, float* pos /*[npairs][B]*/, void* workspace,
                          size_t workspace_bytes, void* stream);
int clipk_simce_grad_pairs(const float* E, int nmod, int B, int P, const int* pairs, const int* reverse, int npairs,
                           const float* scale, const float* lse /*[npairs][B]*/, float w_row, float w_col,
                           float inv_bg, float* dX /*[npairs][B][P]*/, float* dscale_partial /*[npairs][B]*/,
                           void* workspace, size_t workspace_bytes, void* stream);

/* The batched form of the class-aware and of the hard-negative pair: the same npairs <= 6 same-shape problems over
 * E [nmod][B][P], each with the definitions of clipk_simce_{lse,grad}_cls resp. clipk_simce_{lse,grad}_hard for
 * Mx = Ny = B, Nc = 0, label_offset = 0 and cls_x = cls_y = ids[i] - nothing new is defined.  In a PerturbAtlas batch
 * the perturbation and protein rows repeat, one per cell: without ids every row of pert x protein is asked to rank its
 * key above exact copies of it.
 *   ids: HOST array of npairs DEVICE pointers to int64 [B]; an entry may be NULL (that problem: all distinct).  A
 *        problem and its reverse are the two directions of one pair and carry the same pointer (else CLIPK_ERR_BAD_ARG
 *        from the gradient entries).  same_class, eps, beta and the scale are shared by all problems.
 *   upstream: device [npairs] or NULL: the gradient of problem i is multiplied by upstream[i] inside the kernel (the
 *        incoming gradient of the loss the problem belongs to), as clipk_simce_grad_scaled does with its one scalar.
 *   outputs: lse, tgt, cnt, lse_h, pos [npairs][B]; coef [npairs][3][B]; dX [npairs][B][P]; dscale_partial [npairs][B].
 *        grad takes the LSE pass's lse and cnt (cls) resp. coef (hard) whole: problem i reads row i for its queries
 *        and row reverse[i] for its keys.
 * One launch per pass (grid z = problem) plus one finalize each; the key splits are chosen for the whole grid
 * nqb x ksplit x npairs, and their partials merge in a fixed order: deterministic.  No atomics, no allocation, no
 * synchronisation.  P % 4 == 0, P <= 512 (else CLIPK_ERR_UNSUPPORTED); bad pairs / reverse / npairs: CLIPK_ERR_BAD_ARG.
 * workspace: clipk_simce_pairs_cls_workspace resp. clipk_simce_pairs_hard_workspace bytes (each covers both passes). */
size_t clipk_simce_pairs_cls_workspace(int npairs, int B, int P);
int clipk_simce_lse_pairs_cls(const float* E, int nmod, int B, int P, const int* pairs, int npairs, const float* scale,
                              const int64_t* const* ids, int same_class, float eps, float* lse, float* tgt, float* cnt,
                              void* workspace, size_t workspace_bytes, void* stream);
int clipk_simce_grad_pairs_cls(const float* E, int nmod, int B, int P, const int* pairs, const int* reverse, int npairs,
                               const float* scale, const int64_t* const* ids, int same_class, float eps,
                               const float* lse, const float* cnt, float w_row, float w_col, float inv_bg,
                               const float* upstream, float* dX, float* dscale_partial, void* workspace,
                               size_t workspace_bytes, void* stream);
size_t clipk_simce_pairs_hard_workspace(int npairs, int B, int P);
int clipk_simce_lse_pairs_hard(const float* E, int nmod, int B, int P, const int* pairs, int npairs, const float* scale,
                               float beta, const int64_t* const* ids, float* lse_h, float* pos, float* coef,
                               void* workspace, size_t workspace_bytes, void* stream);
int clipk_simce_grad_pairs_hard(const float* E, int nmod, int B, int P, const int* pairs, const int* reverse, int npairs,
                                const float* scale, float beta, const int64_t* const* ids, const float* coef, float w_row,
                                float w_col, float inv_bg, const float* upstream, float* dX, float* dscale_partial,
                                void* workspace, size_t workspace_bytes, void* stream);

/* Materialised logits for the drop-in module API (old/clip.py:67 returns them):
 *   S[Mx,Ny] = scale * X·Y^T, exact f32. */
int clipk_sim_logits(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale,
                     float* S, int64_t lds, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Retrieval over an embedding gallery, exact-f32 MFMA on the tiling of clipk_simce_lse; the logits never reach HBM.
 *   S[i,j] = scale * <X[i,:], Y[j,:]>      (X: Mx queries, Y: Ny gallery rows, P columns; scale is a host float)
 * Order: score descending, equal scores (compared as IEEE values, -0 == +0) by the lower index j.  It is a total order,
 * so results are bitwise independent of the split plan (option retrieval_splits).  Inputs must be finite; with NaN the
 * order is unspecified, but indices stay in [0, Ny).
 * Requirements (both): Mx, Ny, P > 0, P % 4 == 0, X / Y 16-byte aligned; offsets are 64-bit (Ny * P >= 2^31 works).
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED; the workspace helpers return 0 for such shapes.
 *
 * clipk_sim_topk: scores[i, 0..k) / idx[i, 0..k) = the k best (S[i,j], j) of row i in that order; 1 <= k <= 64, k <= Ny.
 * Replaces the full cosine-similarity matrix of run1/full.py:157 followed by a top-k / argmax over it, and
 * logits.argmax(dim=1) at run1/full.py:138,152 (k = 1).  workspace: clipk_sim_topk_workspace(Mx, Ny, P, k) bytes. */
size_t clipk_sim_topk_workspace(int Mx, int Ny, int P, int k);
int clipk_sim_topk(const float* X, int Mx, const float* Y, int Ny, int P, float scale, int k,
                   float* scores /*[Mx,k]*/, int64_t* idx /*[Mx,k]*/, void* workspace, size_t workspace_bytes,
                   void* stream);
/* clipk_sim_rank: rank[i] = #{j != l_i : S[i,j] > S[i,l_i]} + #{j < l_i : S[i,j] == S[i,l_i]}, pos[i] = S[i,l_i], with
 * l_i = labels[i] (device int64 [Mx]) or label_offset + i when labels is NULL (then label_offset >= 0 and
 * label_offset + Mx <= Ny).  rank[i] == 0 exactly when the first-occurrence argmax of row i is l_i: the accuracy
 * (logits.argmax(dim=1) == arange(B)) of run1/full.py:138,152, the confusion-matrix entries of run1/full.py:265.
 * pos has the bits the count compares against.  A device label outside [0, Ny) gives rank -1 and pos NaN.
 * workspace: clipk_sim_rank_workspace(Mx, Ny, P) bytes. */
size_t clipk_sim_rank_workspace(int Mx, int Ny, int P);
int clipk_sim_rank(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const int64_t* labels,
                   int64_t label_offset, int64_t* rank /*[Mx]*/, float* pos /*[Mx]*/, void* workspace,
                   size_t workspace_bytes, void* stream);
/* clipk_sim_rank_cls: the rank among the gallery rows of other classes, cls = device int64 [Ny] gallery class ids:
 *   rank[i] = #{j : cls[j] != cls[l_i] and (S[i,j] > S[i,l_i] or (S[i,j] == S[i,l_i] and j < l_i))}
 * so a duplicate partner of the positive is not a miss.  With all ids distinct it is clipk_sim_rank exactly.
 * workspace: clipk_sim_rank_workspace(Mx, Ny, P) bytes. */
int clipk_sim_rank_cls(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const int64_t* labels,
                       int64_t label_offset, const int64_t* cls, int64_t* rank /*[Mx]*/, float* pos /*[Mx]*/,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Embedding-space diagnostics: one pass over S (same tiles, order and requirements as the retrieval entries above)
 * that keeps the distribution of every row's logits instead of one order statistic.  Replaces the reference's
 * materialise-then-reduce evaluation: the whole cosine_sims matrix of evaluate (run1/full.py:142-160, reduced by
 * .mean() at :253-254), the per-epoch similarity_stats of track_training_dynamics (:401-414), the prediction and
 * confidence logits[i].softmax(0)[p] of analyze_failure_cases (:415-430), the negative difficulty of
 * analyze_hard_negatives_impact (:449-461), and the argmax that feeds the confusion matrix and the per-pair confusion
 * rates (:257-268, :297-306).  (analyze_embedding_collapse, :307-315, needs no pass: diagnostics.group_similarity.)
 *
 * For query i with label l_i (labels[i], device int64 [Mx], or label_offset + i when labels is NULL, as
 * clipk_sim_rank): E_i = { j != l_i : cls_y[j] == cls_x[i] } (cls_x [Mx] / cls_y [Ny] device int64, both or neither;
 * empty without ids: the "mask" rule of clipk_simce_lse_cls), N_i = { j : j != l_i, j not in E_i } the negatives.
 * Per query ([Mx] each):
 *   pos                S[i, l_i], the bits clipk_sim_rank returns
 *   best, best_idx     max of S over {l_i} u N_i, equal scores by the lower index (no ids: clipk_sim_topk, k = 1)
 *   hard, hard_idx     max over N_i alone, same rule; -inf and -1 when N_i is empty
 *   lse                log sum_{{l_i} u N_i} exp S[i,j]: running max / sum per lane, fixed-order merge of the splits
 *   neg_sum, neg_sumsq sum over N_i of S and of S^2, f64
 * Global (int64 [nbins + 2] each, 1 <= nbins <= 256, lo < hi finite, in units of S):
 *   hist_neg           counts of S[i,j] over all i and j in N_i;  hist_pos: the same binning of pos
 * Binning rule: with inv_w = nbins / (hi - lo) evaluated in f64 from the two floats and rounded once to f32,
 *   slot(S) = 0 if S < lo;  nbins + 1 if S >= hi;  else 1 + min(int((S - lo) * inv_w), nbins - 1)
 * with the subtraction and the product in f32 (two roundings, no fused multiply-add) and int() truncating.  One device
 * function bins both histograms.
 * Determinism: pos, best*, hard* and both histograms are bitwise independent of the split plan (option
 * retrieval_splits) and of the run; lse, neg_sum, neg_sumsq are deterministic for a fixed plan and agree across plans
 * to rounding.  A device label outside [0, Ny) gives pos NaN, best_idx = hard_idx = -1 (best = hard = lse = -inf,
 * zero sums) and the row contributes to neither histogram.
 * Accuracy of the sums (u = 2^-24).  Two bounds are stated; the function itself takes any P, the derivation below
 * assumes P <= 4096 (P u <= 2^-12) and Ny < 2^31, and for larger P the bounds are simply not claimed.
 * (1) Guaranteed.  A logit is a k-ordered chain of P fused multiply-adds and one multiplication by scale, so its error
 * is relative to Sabs[i,j] = |scale| sum_p |X[i,p] Y[j,p]|, not to |S[i,j]|: the terms of a dot product can cancel, and
 * no bound in terms of |S| alone holds for every input.  This is a deviation from a bound "c(P) u sum_j |S[i,j]|" and
 * it is meant: Sabs >= |S|, with equality when the products of a row pair share a sign.
 *   |S~ - S| <= (P + 2) u Sabs  (gamma_P = P u / (1 - P u), the product's u, their cross term).
 * A lane adds its 16 values of a tile in f32: <= 15 u sum |S~| (15 additions); the tile partial is converted to f64
 * exactly and everything above it (tiles of a lane, lane halves, key-waves, splits: fewer than Ny / 16 + 2^16 f64
 * additions) costs <= 2^27 2^-53 sum |S~| = u / 4 sum |S~|.  With |S~| <= (1 + 2^-11) Sabs:
 *   |neg_sum[i]   - sum_{N_i} S  | <= (P + 18) u sum_{N_i} Sabs[i,j]
 * The squares are an fma chain (16 roundings per tile) over S~^2, and S~^2 - S^2 = (2 S + e) e with |e| <= (P + 2) u Sabs:
 *   |neg_sumsq[i] - sum_{N_i} S^2| <= (2 P + 24) u sum_{N_i} Sabs[i,j]^2
 * (2) Working bounds of the same constants over |S|, for rows without wholesale cancellation (embeddings):
 *   |neg_sum[i] - sum S| <= (P + 18) u sum_{N_i} |S[i,j]|,   |neg_sumsq[i] - sum S^2| <= (2 P + 24) u sum_{N_i} S[i,j]^2
 * They hold whenever the error of a logit stays below (P + 2) u |S|, which round-to-nearest does on average: the P
 * roundings of a chain act like independent zero-mean errors of size u times a partial sum, i.e. about sqrt(P) u |S|
 * in all.  By the same model the error of a whole row sum is a sum of independent terms bounded by (P + 18) u |S[i,j]|,
 * so it stays below 6 (P + 18) u sqrt(sum_{N_i} S[i,j]^2) except with probability 2 exp(-18) per row (Hoeffding).  A
 * running f32 sum above the tile would instead add about u sqrt(Ny / 192) times the sum itself, which for rows with a
 * non-zero mean is far above that figure; the GPU tests assert (1), (2) and this last one.
 * None of the bounds has a term that grows with Ny.
 * Never allocates, never synchronises, capturable.  workspace (16-byte aligned): clipk_sim_stats_workspace(Mx, Ny, P,
 * nbins) bytes, 0 for refused shapes. */
size_t clipk_sim_stats_workspace(int Mx, int Ny, int P, int nbins);
int clipk_sim_stats(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const int64_t* labels,
                    int64_t label_offset, const int64_t* cls_x, const int64_t* cls_y, int nbins, float lo, float hi,
                    float* pos /*[Mx]*/, float* best /*[Mx]*/, int64_t* best_idx /*[Mx]*/, float* hard /*[Mx]*/,
                    int64_t* hard_idx /*[Mx]*/, float* lse /*[Mx]*/, double* neg_sum /*[Mx]*/,
                    double* neg_sumsq /*[Mx]*/, int64_t* hist_neg /*[nbins+2]*/, int64_t* hist_pos /*[nbins+2]*/,
                    void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prefiltered exact top-k: the results of clipk_sim_topk, bit for bit, with the bulk of the similarity work on the bf16
 * matrix pipe (v_mfma_f32_32x32x16_bf16) instead of the exact-f32 one.  Replaces the same reference sites as
 * clipk_sim_topk (the similarity matrix of run1/full.py:157 and the argmax of run1/full.py:138,152).
 *   1. clipk_split_bf16 once per gallery (incrementally as rows are added): bf16 plane(s) and max_j |Y_j|.
 *   2. clipk_sim_topk_cand: the approximate top-kc of every query, A[i,j] = scale * <X_i, Y_j>_bf16.
 *   3. clipk_sim_rerank: the exact scores of those kc keys (the bits clipk_sim_topk computes), their top k, and a
 *      certificate per query; 4. the caller runs clipk_sim_topk on the uncertified rows and scatters them back.
 * Modes: one plane (bf16: A = sum hi(x) hi(y)) or two (bf16x3: x = hi + lo + r, lo = bf16(x - hi),
 * A = sum hi.hi + hi.lo + lo.hi).  Planes: row pitch PP = P rounded up to a multiple of 32 bf16 elements, pads zero.
 * Requirements (all three): P % 4 == 0, P <= 65536 (else CLIPK_ERR_UNSUPPORTED), 16-byte aligned pointers.
 *
 * Certificate.  With c the kc-th (weakest) approximate candidate score and t_k the k-th exact score among the
 * candidates, query i is certified when t_k > c + eps_i, where eps_i bounds |A[i,j] - S[i,j]| for every key j:
 *   eps_i = |scale| |X_i| max_j|Y_j| eps_rel + eps_abs.
 * Every non-candidate j has A[i,j] <= c, so S[i,j] <= c + eps_i < t_k: it is below k candidates and cannot enter the
 * top k; the order among candidates is the exact one.  A query whose list holds every key (Ny <= kc) is certified
 * trivially.  The comparison is made in f64 with eps_i enlarged by (1 + 2^-30), which covers the roundings of its own
 * evaluation; |X_i| is summed in f64 and |Y|max is rounded upward to f32.  Non-finite results, NaN scores, norms with
 * |scale| |X_i| |Y|max >= 2^126 (where f32 partial sums could overflow) and short lists are never certified.
 * eps_rel (u = 2^-24, v = 2^-8 the unit roundoffs of f32 and bf16 - bf16 keeps 8 significant bits, so a single rounding
 * moves a value by up to 2^-8 of it, not 2^-9; every term bounds an error relative to sum_p |x_p y_p| <= |x| |y|):
 *   operands, bf16:   |hi(x) hi(y) - x y| <= (2v + v^2) |x y|
 *   operands, bf16x3: |hi lo| <= v(1 + v)|x|, |r| <= v^2 |x|; the dropped lo.lo + hi.r + r.hi + lo.r + r.lo + r.r
 *                     sum to <= (3 v^2 + 6 v^3 + 4 v^4) |x y| <= (3 v^2 + 7 v^3) |x y|
 *   bf16 MFMA accumulation: its order and rounding are not documented.  The products of bf16 operands are exact in
 *                     f32; n = P (bf16) or 3P (bf16x3) of them are summed.  Taken as gamma = n 2^-22 (four times the
 *                     n u of f32 round-to-nearest in any order) times their magnitude, (1 + v)^2 (bf16) or
 *                     (1 + v)^2 (1 + 2v) (bf16x3) times sum |x y|.  The GPU tests measure |A - S| <= eps_i / 2.
 *   the exact f32 kernel: a chain of P fused multiply-adds, <= P u / (1 - P u) <= P 2^-23
 *   the two multiplications by scale: <= 2^-22
 * eps_abs = (|scale| P (|X_i| + |Y|max + 1) + 1) 2^-120 covers subnormals: the conversion and the MFMA may flush
 * subnormal operands (the lo plane produces them) and results to zero, each such flush moving a product or a partial sum
 * by less than 2^-126 (|Y| + 1) per term.  retrieval.prefilter_eps_rel(P, mode) evaluates eps_rel.
 *
 * clipk_split_bf16: hi[n_rows, PP] = bf16(X) (round to nearest even), lo (NULL: one plane) = bf16(X - hi), pads zero;
 * norm_max (device f32 [1], NULL: not tracked) = max(*norm_max, |X_r| rounded upward), +inf for NaN or huge rows. */
int clipk_split_bf16(const float* X, int n_rows, int P, void* hi, void* lo, float* norm_max, void* stream);
/* clipk_sim_topk_cand: cand_scores / cand_idx [Mx, kc] = the kc best (A[i,j], j) of row i in the clipk_sim_topk order
 * applied to A; 1 <= kc <= 64.  Yhi / Ylo: the gallery's planes (Ylo NULL: bf16 mode).  When Ny < kc the list ends in
 * fillers with score -inf.  The queries are split into the workspace: clipk_sim_topk_cand_workspace(Mx, Ny, P, kc,
 * planes) bytes, planes = 1 or 2. */
size_t clipk_sim_topk_cand_workspace(int Mx, int Ny, int P, int kc, int planes);
int clipk_sim_topk_cand(const float* X, int Mx, const void* Yhi, const void* Ylo, int Ny, int P, float scale, int kc,
                        float* cand_scores /*[Mx,kc]*/, int64_t* cand_idx /*[Mx,kc]*/, void* workspace,
                        size_t workspace_bytes, void* stream);
/* clipk_sim_rerank: scores / idx [Mx, k] = the k best candidates of row i by their exact scores S[i,j] (the bits of
 * clipk_sim_topk), in its order; certified[i] (int32) = 1 when those are the top k of the whole gallery by the bound
 * above, else 0 (then scores / idx of that row are unspecified).  1 <= k <= kc <= 64, k <= Ny; eps_rel in [0, 1);
 * y_norm_max: device f32 [1], an upper bound of every |Y_j| (clipk_split_bf16's).  No workspace. */
int clipk_sim_rerank(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const int64_t* cand_idx,
                     const float* cand_scores, int kc, int k, double eps_rel, const float* y_norm_max,
                     float* scores /*[Mx,k]*/, int64_t* idx /*[Mx,k]*/, int* certified /*[Mx]*/, void* stream);

/* Cross-entropy on MATERIALISED logits — the reference's loss call sites take the logits tensor its modules return:
 * F.cross_entropy(logits, arange(B)) at old/ablation.py:16 / run1/full.py:133, the symmetric pair at
 * current/rna_clip_codes.ipynb:1952-1953, and (F.cross_entropy(cat([S, S_cache], 1)) + F.cross_entropy(S^T)) / 2
 * at old/clip_opt.py:130-151.  (Training should use clipk_simce_*: there the logits never reach HBM.)
 *   lse:  columns == 0: lse[i] = logsumexp_j [S | S2][i, j], pos[i] = S[i, i + label_offset]          (i < M)
 *         columns == 1: lse[j] = logsumexp_i S[i, j],        pos[j] = S[j + label_offset, j]          (j < N; N2 == 0)
 *   bwd:  dS[i,j]  = g * ( w_row (exp(S_ij - lse_row[i]) - [j == i + off_row])
 *                        + w_col (exp(S_ij - lse_col[j]) - [i == j + off_col]) ),
 *         dS2[i,j] = g * w_row exp(S2_ij - lse_row[i]);   lse_row / lse_col may be NULL (direction unused);
 *         w_row / w_col carry the 1 / batch factors; g = device scalar (upstream gradient).
 * A label outside the matrix gives pos = 0 and no one-hot.  A -inf logit is a zero term: it adds nothing to lse, a row
 * or column without a finite logit has lse = -inf (torch.logsumexp), and no NaN comes out unless one went in (the
 * backward of an all--inf row is exp(-inf + inf): leave such rows out).  ld / ld2 / ldd / ldd2 are row strides in
 * elements.  columns == 1 with N2 > 0 is CLIPK_ERR_UNSUPPORTED.  Every M, N, N2 that fits an int is accepted by both
 * entry points: the backward walks its rows with a grid-stride loop over at most 65 535 grid rows. */
int clipk_ce_logits_lse(const float* S, int64_t ld, int M, int N, const float* S2, int64_t ld2, int N2,
                        int columns, int label_offset, float* lse, float* pos, void* stream);
int clipk_ce_logits_bwd(const float* S, int64_t ld, int M, int N, const float* S2, int64_t ld2, int N2,
                        const float* lse_row, const float* lse_col, float w_row, float w_col,
                        int label_offset_row, int label_offset_col, const float* gscale,
                        float* dS, int64_t ldd, float* dS2, int64_t ldd2, void* stream);

/* Linear + cross-entropy against INTEGER labels, exact f32 (v_mfma_f32_16x16x4_f32, classes padded to the 16-wide tile):
 * the last layer and the loss of every classifier head of old/classifier.py (nn.Linear(h, num_classes) at :14,31,40,52
 * under nn.CrossEntropyLoss()(logits, labels) at old/ablation.py:30 and torch.max(logits, 1) at :45).
 *   Z[i,c] = sum_{k<K1} X1[i,k] W[c,k] + sum_{k<K2} X2[i,k] W[c,K1+k] + bias[c]          i < M, c < C
 * X1 [M,K1], X2 [M,K2] contiguous; X2 == NULL together with K2 == 0 is a single input, two inputs are the
 * torch.cat([rna_embeds, protein_embeds], -1) of old/ablation.py:29,44 without the concatenation.  W [C, K1+K2] is the
 * nn.Linear weight, bias [C] may be NULL, labels device int64 [M].
 * fwd, one pass over X: lse[i] = logsumexp_c Z[i,c]; tgt[i] = Z[i, labels[i]]; pred[i] = the first-occurrence argmax of
 *   row i (equal logits: the lower class, torch.max(logits, 1)'s rule); logits[i * ldz + c] = Z[i,c] if logits != NULL.
 *   Each of lse / tgt / pred / logits may be NULL (not all); labels may be NULL when tgt is.  The mean loss is
 *   clipk_ce_combine(lse, tgt, NULL, NULL, M, 1, 0, M).  No workspace.
 * bwd: with G[i,c] = g[0] / M * (exp(Z[i,c] - lse[i]) - [c == labels[i]]) (g: device scalar, the upstream gradient; Z
 *   recomputed with the forward's bits): dW[C,K] (+)= G^T [X1|X2], dbias[C] (+)= sum_i G, dX1 = G W[:, :K1],
 *   dX2 = G W[:, K1:], each written only where its pointer is non-NULL (not all NULL); accumulate != 0 adds into dW /
 *   dbias (a parameter's .grad) as clipk_gemm_wgrad_f32 does.  The cross-workgroup partial sums of dW / dbias go to the
 *   workspace and are added in split order by a last kernel: no float atomics, bitwise reproducible run to run.
 *   DEVIATION from "one pass": G needs a row's whole contraction before any of dW can be formed.  An X tile could wait
 *   in LDS (32 rows x 1024 f32 = 128 of 160 KiB), but the dW partial (C x K f32: 256 KiB at C = 64, K = 1024, up to 1 MiB)
 *   would have to stay in the registers of the one workgroup that tile leaves room for, which holds only for C <= 16,
 *   K <= 1024.  So the backward reads X twice at every shape: once for Z -> G (G [M, 16 ceil(C/16)]
 *   goes to the workspace), once for G^T X.
 * A label outside [0, C): tgt = NaN (so the loss is NaN), the row adds nothing to any gradient (its dX rows are zero),
 * pred is still valid; nothing is read or written out of bounds.
 * Supported: 1 <= C <= 64, K1 % 4 == 0, K2 % 4 == 0, K1 + K2 <= 4096, M >= 1, X1 / X2 / W / dW / dX / workspace 16-byte
 * aligned; anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED, and clipk_linear_ce_workspace returns 0.
 * Never allocates, never synchronises, capturable.  workspace (bwd only): clipk_linear_ce_workspace(M, K1, K2, C) bytes.
 * Accuracy (u = 2^-24): a logit is a chain of K fused multiply-adds in a fixed permutation of k and one addition of the
 * bias: |Z~ - Z| <= (K + 4) u (sum_k |x_k w_k| + |b|); lse and tgt carry that error plus a few u of expf / logf.
 * What bounds it (measured on an MI355X at M = 131072, K = 1024; record: profiles/probe/README.md): at C = 16 the X
 * stream - the forward reads X at 3.9 TB/s, 63 % of the HBM copy rate, with the f32 matrix pipe at 20 % of its peak.  At
 * C = 64 neither is saturated (1.8 TB/s, 59 of 155 TFLOP/s): per 16 rows x 16 columns of X a wave issues 4 ceil(C/16)
 * MFMAs and re-reads ceil(C/16) float4s of W from cache, and that traffic and the unpipelined loop bind before the
 * roughly balanced X stream and matrix pipe of the model do. */
size_t clipk_linear_ce_workspace(int M, int K1, int K2, int C);
int clipk_linear_ce_fwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                        const int64_t* labels, int M, int C, float* lse /*[M]*/, float* tgt /*[M]*/,
                        int64_t* pred /*[M]*/, float* logits, int64_t ldz, void* stream);
int clipk_linear_ce_bwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                        const int64_t* labels, int M, int C, const float* lse, const float* g, int accumulate,
                        float* dW /*[C,K1+K2]*/, float* dbias /*[C]*/, float* dX1 /*[M,K1]*/, float* dX2 /*[M,K2]*/,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The same Linear + cross-entropy for ANY class count: 1 <= C <= 65536.  The reference's own probe task is far past 64
 * classes - run1/proposal.MD:3 pairs 2,547 immune cell types with 158 unique markers, and every head takes num_classes as
 * a free argument (old/classifier.py:14,31,40,52; old/ablation.py:30,45).  Definitions of Z, lse, tgt, pred, G, dW, dbias,
 * dX1, dX2, the out-of-range-label rule and the accumulate flag: exactly those of clipk_linear_ce_* above.  No logits
 * output (clipk_gemm_f32 serves logits); each of lse / tgt / pred may be NULL (not all).
 * fwd: a workgroup owns 64 rows of [X1|X2] and walks 64-class tiles of W on v_mfma_f32_32x32x2_f32 (classes on the MFMA
 *   rows, X rows on the lanes; the second source continues the first one's accumulator), keeping per row the running
 *   (max, sum), the best (value, class) and the target logit.  Equal logits resolve to the lower class also across class
 *   tiles and splits: the merge rule "larger value, then lower class" is associative.  The class range is split across
 *   workgroups when M alone does not fill the chip; the partials [split][M][5] go to the workspace and a second kernel
 *   merges them in split order.
 * bwd: the forward's kernel recomputes Z with the forward's bits and writes G to the workspace (pitch C rounded up to 4,
 *   zeros in the padding); dW and dbias are summed over row splits and 64-class groups by the weight-gradient kernel that
 *   clipk_linear_ce_bwd runs too (csrc/linear_ce_bwd.h) and the splits are added in split order (clipk_gemm_f32 does not split its contraction, here the M rows: at
 *   C = 158 it ran 24 workgroups); dX comes from clipk_gemm_f32 on G, one call per source.  The rows are processed in
 *   slabs whose G stays at 128 MiB or less (half of the Infinity Cache); dW / dbias accumulate over the slabs in slab
 *   order (record of the slab A/B: profiles/probe/README.md).
 * Supported: M >= 1, 1 <= C <= 65536, K1 % 4 == 0, K2 % 4 == 0, K1 >= 4, K1 + K2 <= 4096, X1 / X2 / W / dW / dX / workspace
 * 16-byte aligned; anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED and the workspace helper returns 0.
 * Never allocates, never synchronises, capturable, no float atomics: results depend on the shapes alone.  workspace (fwd
 * and bwd): clipk_linear_ce_tiled_workspace(M, K1, K2, C) bytes.
 * Accuracy: the bounds of clipk_linear_ce_* hold (a logit is a chain of K fused multiply-adds, k ascending per source,
 * and the bias addition); bits differ from clipk_linear_ce_* at C <= 64, which keeps its own kernels. */
size_t clipk_linear_ce_tiled_workspace(int M, int K1, int K2, int C);
int clipk_linear_ce_tiled_fwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                              const int64_t* labels, int M, int C, float* lse /*[M]*/, float* tgt /*[M]*/,
                              int64_t* pred /*[M]*/, void* workspace, size_t workspace_bytes, void* stream);
int clipk_linear_ce_tiled_bwd(const float* X1, int K1, const float* X2, int K2, const float* W, const float* bias,
                              const int64_t* labels, int M, int C, const float* lse, const float* g, int accumulate,
                              float* dW /*[C,K1+K2]*/, float* dbias /*[C]*/, float* dX1 /*[M,K1]*/, float* dX2 /*[M,K2]*/,
                              void* workspace, size_t workspace_bytes, void* stream);

/* out[cols, rows] = scale_dev[0] * in[rows, cols]^T (f32; scale_dev NULL = 1).  Operand preparation of the exact-f32
 * products that differentiate the materialised logits (d/dA = scale * dS · B, d/dB = scale * dS^T · A of
 * old/clip.py:67) and of the ICNN's transposed weights (triple_flow/2_icnn_core.py:181-211).  One f32 rounding per
 * element (a copy without a scale); any rows / cols: the row tiles beyond grid y's 65 535 are walked by a loop. */
int clipk_transpose_scale_f32(const float* in, int rows, int cols, const float* scale_dev, float* out, void* stream);

/* Exact-f32 Linear for the ICNN transport maps (the reference forces f32 there: triple_flow/2_icnn_core.py:195):
 *   out[M,N] = X[M,K] · W[N,K]^T (+ bias[N]) (+ addend_scale[0] * addend[M,N])
 * Replaces self.linear(x) + scale * F.linear(z, softplus(W+)) at triple_flow/2_icnn_core.py:102-119 and the
 * matching products of the analytic input gradient T(x) = dPsi/dx (:181-211).  Same f32-MFMA kernel as
 * clipk_sim_logits.  K % 4 == 0, K <= 768. */
int clipk_gemm_f32_nt(const float* X, int M, const float* W, int N, int K, const float* bias,
                      const float* addend, const float* addend_scale /* device scalar or NULL (=1) */,
                      float* out, void* stream);

/* Tiled exact-f32 GEMM (v_mfma_f32_32x32x2_f32, 128 x 64 tiles, LDS-staged) with all four operand layouts:
 *   out[M,N] = alpha[0] * opA(A) · opB(B) (+ bias[N]) (+ addend_scale[0] * addend[M,N])     (alpha NULL = 1)
 *   transA == 0: A is [M,K] (lda);  transA == 1: A is stored [K,M] (contraction-major: dW = dY^T X)
 *   transB == 0: B is [N,K] (nn.Linear weight, out = A·B^T);  transB == 1: B is stored [K,N] (dA = dZ · W)
 * Every product of the ICNN potential, of its input gradient T(x) = dPsi/dx and of the training path's double backward
 * (triple_flow/2_icnn_core.py:102-119,181-211 under autocast(enabled=False)), and the gradients of the materialised
 * logits (old/clip.py:67): no transposed copies, any K.  lda / ldb % 4 == 0, A / B 16-byte aligned.
 * M <= 64 rows against a large weight (K >= 256, A not transposed: forward and input gradient of every Linear of the
 * position-0-sliced notebook models, M = batch) take the skinny form: one bandwidth-bound pass over B, the contraction
 * split 16 ways inside a workgroup and - given a workspace - across workgroups so that every CU streams its share.
 * workspace: clipk_gemm_f32_workspace(...) bytes (0 = none needed; scratch for the partial tiles of a split launch, summed
 * in split order by a second kernel); NULL or too small: no cross-workgroup split. */
size_t clipk_gemm_f32_workspace(int M, int N, int K, int transA, int transB);
int clipk_gemm_f32(const float* A, int64_t lda, int transA, const float* B, int64_t ldb, int transB,
                   int M, int N, int K, const float* alpha /* device scalar or NULL */, const float* bias,
                   const float* addend, int64_t ldadd, const float* addend_scale /* device scalar or NULL (=1) */,
                   float* out, int64_t ldo, void* workspace, size_t workspace_bytes, void* stream);

/* out[c] (+)= sum_r x[r][c] (x f32 [rows, cols] contiguous): the bias gradient dY.sum(0) of the exact-f32 Linear layers
 * (old/clip.py:11,27,31 under autograd), accumulated straight into the parameter's .grad; fixed summation order. */
int clipk_colsum_f32(const float* x, int rows, int cols, float* out, int accumulate, void* stream);
/* Deferred parameter gradients of several LayerNorms in one launch.  clipk_layernorm_bwd called with dgamma = dbeta = NULL
 * leaves its per-block partial rows [blocks][2][cols] (blocks = clipk_layernorm_bwd_workspace(rows, cols) / (2 cols 4)) in the
 * workspace it was given; with one such buffer per LayerNorm, this reduces all of them - what nn.LayerNorm's weight.grad /
 * bias.grad receive from autograd (old/clip.py:12,28,32; rna_clip_codes.ipynb:1911-1923) - when the backward pass is over:
 * desc_dev = n x 6 int64 in device memory {partial rows, blocks, cols, dgamma, dbeta, accumulate}; max_cols = the widest. */
int clipk_colreduce_batched(const int64_t* desc_dev, int n, int max_cols, void* stream);

/* Both parameter gradients of an exact-f32 Linear in one call: dW[N, K] (+)= dY[M, N]^T X[M, K], dbias[N] (+)= dY.sum(0)
 * (what autograd computes for nn.Linear under the reference's fp32 callers: old/clip.py:11,27,31; the Linear layers of
 * RNARBPCLIPModel / ContrastiveModel, current/rna_clip_codes.ipynb:1911-1954) - the f32 sibling of clipk_gemm_wgrad.
 * dW or dbias may be NULL (not both).  accumulate != 0 adds into dW / dbias (a parameter's .grad).  M <= 64 (the models
 * sliced to the one position they pool: M = batch rows): ONE launch, one pass over dW with dbias from the same operand
 * registers; more rows (or dbias alone): the tiled clipk_gemm_f32 (contraction-major operands) + clipk_colsum_f32, which
 * needs lddy == N: dbias with another lddy is CLIPK_ERR_UNSUPPORTED there, refused before anything is launched (dW untouched).
 * dW is bit-identical to clipk_gemm_f32(dY, transA = 1, X, transB = 1, addend = dW) either way. */
int clipk_gemm_wgrad_f32(const float* dY, int64_t lddy, const float* X, int64_t ldx, float* dW, int64_t lddw,
                         float* dbias, int M, int N, int K, int accumulate, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row-wise normalisation kernels (one wave per row, f32 statistics).
 * LayerNorm forward:  y = (x-mean)*rstd*gamma + beta, optional activation fused after it
 * (old/clip.py:12,28-29,32; transformer / ESM LayerNorms).  x is f32 or bf16; writes any of
 * y_f32 / y_bf16 (NULL to skip) and mean/rstd [rows] for the backward.
 */
int clipk_layernorm_fwd(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta,
                        float eps, int act, float* y_f32, void* y_bf16, int64_t ldy,
                        float* mean, float* rstd, int rows, int cols, void* stream);
/* LayerNorm backward: dx (f32 and/or bf16), and per-block partial dgamma/dbeta in workspace followed
 * by a deterministic column reduce into dgamma/dbeta (accumulate flag as above).  If act != NONE the
 * incoming dy is first multiplied by act'(ln_out) where ln_out is recomputed from x, mean, rstd.
 * dx_add: optional [rows,cols] f32 or bf16 (dx_add_dtype) added to the result (residual-stream gradient).
 * drop_p > 0: the bf16 output (only) is multiplied by the dropout mask keep(drop_seed, row * cols + col) / (1 - p): it is
 * the gradient of the dropped-out Linear output that was added to the residual stream in front of this LayerNorm
 * (dropout1 / dropout2 of nn.TransformerEncoderLayer); the f32 output stays the residual-path gradient.
 * dgamma == dbeta == NULL: input gradient only. */
size_t clipk_layernorm_bwd_workspace(int rows, int cols);
int clipk_layernorm_bwd(const void* dy, int dy_dtype, int64_t lddy, const void* x, int x_dtype, int64_t ldx,
                        const float* gamma, const float* beta, const float* mean, const float* rstd, int act,
                        const void* dx_add, int dx_add_dtype, float* dx_f32, void* dx_bf16, int64_t lddx,
                        float* dgamma, float* dbeta, int accumulate,
                        int rows, int cols, float drop_p, uint32_t drop_seed, void* workspace, size_t workspace_bytes, void* stream);

/* Backward OF clipk_layernorm_bwd (second order), f32: the ICNN transport map is T(x) = dPsi/dx
 * (triple_flow/2_icnn_core.py:181-211: torch.autograd.grad(..., create_graph=True)) and the training loss of
 * triple_flow/4_transport_maps.py:113-145 is a function of T, so autograd differentiates the first backward
 *   da = LNact_bwd(dy; a, gamma, beta)   (what clipk_layernorm_bwd computes, act in {NONE, CELU, SOFTPLUS})
 * with respect to dy, a, gamma and beta.  g = cotangent of da [rows, cols]; outputs d_dy, d_a [rows, cols] (either may
 * be NULL) and d_gamma / d_beta [cols] (both or neither; overwritten or accumulated).  mean / rstd as saved by
 * clipk_layernorm_fwd for `a`.  One leading dimension ld for g, dy, a, d_dy, d_a.  workspace:
 * clipk_layernorm_bwd_workspace(rows, cols) bytes. */
int clipk_layernorm_bwd2(const float* g, const float* dy, const float* a, int64_t ld, const float* gamma,
                         const float* beta, const float* mean, const float* rstd, int act, float* d_dy, float* d_a,
                         float* d_gamma, float* d_beta, int accumulate, int rows, int cols,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Final LayerNorm of an encoder + masked mean over the L token rows of each sample in one pass: pooled[b] =
 * mean_{l valid} LN(x[b, l]) (the pooling of run1/configuration_hybrid_clip.py:109,148 `use_mean_pooling`, fair-esm
 * mean over residues current/tf_clip_codes (1).ipynb:1188, behind the encoders' last LayerNorm modeling_esm.py:552-553 /
 * rna_clip_codes.ipynb:1923).  The normalised rows are never written.  x f32 or bf16 [B*L, cols], mask u8 [B*L] (1 = valid) or
 * NULL; outputs pooled f32 [B, cols], mean / rstd f32 [B*L] (for the backward; the bits clipk_layernorm_fwd gives for the
 * same rows, at every width), row_weight f32 [B*L] = the row's weight in its sample's mean (1 / #valid rows, 0 for a masked
 * row or an empty sample).
 * Backward: row r gets dy = dpooled[r / L] * row_weight[r] and goes through the LayerNorm backward
 * (outputs / workspace / dgamma / dbeta as clipk_layernorm_bwd, workspace size clipk_layernorm_bwd_workspace(B*L, cols)). */
int clipk_layernorm_meanpool_fwd(const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* beta, float eps,
                                 const uint8_t* mask, int B, int L, int cols, float* pooled, float* mean, float* rstd,
                                 float* row_weight, void* stream);
int clipk_layernorm_meanpool_bwd(const float* dpooled, const float* row_weight, int B, int L,
                                 const void* x, int x_dtype, int64_t ldx, const float* gamma, const float* mean, const float* rstd,
                                 float* dx_f32, void* dx_bf16, int64_t lddx, float* dgamma, float* dbeta, int accumulate,
                                 int cols, void* workspace, size_t workspace_bytes, void* stream);

/* F.normalize(x, dim=-1) with eps=1e-12 (old/clip.py:63-64): y = x / max(||x||, eps); f32. */
int clipk_l2norm_fwd(const float* x, float* y, float* norm, int rows, int cols, float eps, void* stream);
int clipk_l2norm_bwd(const float* dy, const float* y, const float* norm, float* dx,
                     int rows, int cols, float eps, void* stream);

/* Elementwise helpers on f32/bf16 buffers (n elements, n % 8 == 0 not required). */
int clipk_cast_f32_to_bf16(const float* x, void* y, int64_t n, void* stream);
int clipk_cast_bf16_to_f32(const void* x, float* y, int64_t n, void* stream);
/* W f32 [rows,cols] -> bf16 copy and bf16 transposed copy [cols,rows] (either may be NULL).
 * il_rows > 0: rows [0, il_rows) of both copies are written in PAIR-INTERLEAVED head order for heads of il_hd rows - copy
 * row 2 j (+1) of a head holds W row j (+ il_hd / 2) of that head - the order in which clipk_gemm_nt's interleaved RoPE
 * epilogue (rope_interleaved) expects the q and k sections of ESM-2's fused qkv projection (modeling_esm.py:362-374).
 * rows <= 64 * 65 535 (one 64-row tile per grid row), else CLIPK_ERR_UNSUPPORTED before any launch; the batched entry
 * below has no such limit. */
int clipk_cast_transpose(const float* w, void* w_bf16, void* wt_bf16, int rows, int cols, int il_hd, int il_rows, void* stream);
/* The same for n weights in one launch (what `optimizer.step()` leaves to do before the next forward: the reference
 * re-reads its f32 nn.Linear weights under autocast every step, old/clip.py:11).  desc_dev: device array of n
 * records {w, w_bf16, wt_bf16, rows, cols, il_hd, il_rows}, seven int64 each (pointers as integers, either output may be 0). */
int clipk_cast_transpose_batched(const void* desc_dev, int n, void* stream);
/* y = act(x) / dx = dy * act'(x) on f32. */
int clipk_act_fwd(const float* x, float* y, int act, int64_t n, void* stream);
int clipk_act_bwd(const float* dy, const float* x, float* dx, int act, int64_t n, void* stream);
/* out_bf16 = dy * act'(aux_bf16): activation backward between two Linear layers; dy f32 or bf16. */
int clipk_dact(const void* dy, int dy_dtype, const void* aux_bf16, int act, void* out_bf16, int64_t n, void* stream);
/* y = a + s[0] * b  (skip + layer_scale * projected, old/clip_opt.py:41-44), f32; a == NULL: y = s[0] * b (its backward). */
int clipk_axpby_dev(const float* a, const float* b, const float* s, float* y, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-head self-attention, flash style (no LxL matrix in HBM), bf16 MFMA, f32 softmax.
 * qkv: bf16 [B*L, 3*H*D] rows = tokens (b-major), columns = [q heads | k heads | v heads];
 * key_mask: uint8 [B, L], 1 = valid key, or NULL; rope_cos/sin: f32 [L, D/2] or NULL (ESM-2 rotary,
 * rotate-half, applied to q and k after q *= q_scale — transformers modeling_esm.py:48-52,74-79,374);
 * out: bf16 [B*L, H*D]; lse: f32 [B, H, L] (log-sum-exp of the scaled scores, saved for backward).
 * Replaces nn.MultiheadAttention inside nn.TransformerEncoderLayer (rna_clip_codes.ipynb:1915) and
 * EsmSelfAttention (modeling_esm.py:306-314,362-384).  D in {8..160}, D % 8 == 0.
 * dropout_p > 0: dropout on the attention probabilities (P~ = P * keep / (1 - p) feeds P·V, the normaliser uses P),
 * mask = hash(dropout_seed, ((token row * H + h) * L + key)); pass the same (p, seed) to the backward.
 */
int clipk_attn_fwd(const void* qkv, const uint8_t* key_mask, const float* rope_cos, const float* rope_sin,
                   void* out, float* lse, int B, int L, int H, int D, float q_scale, float dropout_p,
                   uint32_t dropout_seed, void* stream);
/* Backward: dqkv bf16 [B*L, 3*H*D] from dout bf16 [B*L, H*D]; recomputes P from qkv + lse.
 * delta: f32 [B,H,L] provided by the caller; the backward writes delta = rowsum(dout * out) of the stored bf16 `out` there.
 * A sequence with no valid key (key_mask all zero): clipk_attn_fwd gives zero `out` rows and lse = -inf, and the backward
 * gives zero dqkv rows (and delta = 0) for it - no NaN - whatever kernel the shape and the options select; `dout` is not
 * read as zero at masked positions: a key mask hides keys, not queries.
 * prerotated: 0 = q / k in qkv are un-rotated (the kernels rotate at staging when given tables); 1 = already rotated
 * (clipk_rope_qk / clipk_attn_fwd_rot / clipk_gemm_nt's RoPE epilogue), rotate-half column order; 2 = already rotated, heads in
 * PAIR-INTERLEAVED column order (clipk_gemm_nt rope_interleaved): the gradients leave through the matching RoPE^T. */
int clipk_attn_bwd(const void* qkv, const uint8_t* key_mask, const float* rope_cos, const float* rope_sin,
                   const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                   int B, int L, int H, int D, float q_scale, int prerotated, float dropout_p, uint32_t dropout_seed,
                   void* stream);
/* Rotate-half RoPE (transformers modeling_esm.py:88-110) applied ONCE, in place, to the q and k sections of
 * qkv bf16 [B*L, 3*H*D].  Afterwards call clipk_attn_fwd WITHOUT rope tables and clipk_attn_bwd with the tables and
 * prerotated = 1: q / k are then staged as they are and only the gradients go through RoPE^T. */
int clipk_rope_qk(void* qkv, const float* rope_cos, const float* rope_sin, int B, int L, int H, int D, void* stream);
/* clipk_rope_qk followed by clipk_attn_fwd(rope = NULL) in one call: q / k in `qkv` are rotated IN PLACE and the
 * attention output / lse computed from the rotated values (same bits as the two calls).  Short heads (D in
 * {16, 24, 32}, 128 < L <= 256) do both in one kernel - one workgroup owns every row of a head, rotates it while
 * staging and writes it back; other shapes make the two calls.  Backward: clipk_attn_bwd(..., prerotated = 1). */
int clipk_attn_fwd_rot(void* qkv, const uint8_t* key_mask, const float* rope_cos, const float* rope_sin,
                       void* out, float* lse, int B, int L, int H, int D, float q_scale, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact-f32 multi-head self-attention (f32 q / k / v, f32 scores, f32 softmax, f32 P·V; VALU fmas in a fixed order) for
 * the models the reference runs WITHOUT autocast: nn.MultiheadAttention inside the nn.TransformerEncoderLayer stacks of
 * RNARBPCLIPModel (current/rna_clip_codes.ipynb:1911-1954) and of the tri-modal ContrastiveModel
 * (current/tf_clip_codes (1).ipynb:13056-13072,13113-13176).  Layouts as clipk_attn_fwd / clipk_attn_bwd with f32
 * tensors: qkv [B*L, 3*H*D], out / dout [B*L, H*D], dqkv [B*L, 3*H*D], lse / delta [B, H, L]; key_mask u8 [B, L]
 * (1 = valid) or NULL; same dropout mask (hash, element index) as the bf16 kernels.  Any D in 1..192 (no multiple-of-8
 * rule: the notebook's 120 / 8 = 15 runs unpadded).  A row whose keys are all masked gives a zero output row and
 * lse = -inf, as clipk_attn_fwd. */
int clipk_attn_f32_fwd(const float* qkv, const uint8_t* key_mask, float* out, float* lse, int B, int L, int H, int D,
                       float q_scale, float dropout_p, uint32_t dropout_seed, void* stream);
int clipk_attn_f32_bwd(const float* qkv, const uint8_t* key_mask, const float* out, const float* dout, const float* lse,
                       float* delta /* scratch [B,H,L] */, float* dqkv, int B, int L, int H, int D, float q_scale,
                       float dropout_p, uint32_t dropout_seed, void* stream);
/* y[i] = x[i] * keep(seed, i) / (1 - p) (+ addend[i]): nn.Dropout on an f32 tensor (out_proj / linear2 outputs in front
 * of their residual add, the FFN activation: nn.TransformerEncoderLayer(dropout = p), rna_clip_codes.ipynb:1915) with
 * the counter-based mask of the GEMM epilogues (element index = row-major position); the backward is the same call on
 * the gradient.  addend may be NULL; y may alias x. */
int clipk_dropout_f32(const float* x, const float* addend, float* y, int64_t n, float p, uint32_t seed, void* stream);
/* Dropout under hipGraph replay (training.GraphedTrainStep with nn.TransformerEncoderLayer's dropout = 0.1 active,
 * rna_clip_codes.ipynb:1915, :2061-2089): a captured launch carries its seed as a constant, so every replay would repeat
 * the mask.  While a device word is registered here, EVERY dropout site of the library (clipk_gemm_nt's drop_p,
 * clipk_attn_*'s dropout_p, clipk_attn_f32_*, clipk_dropout_f32, clipk_layernorm_bwd's drop_p) uses
 * seed + *epoch_dev * 0x9E3779B9 instead of seed, read when the kernel RUNS: the captured step increments the word once per
 * replay, after its backward (which re-draws the forward's masks from the same seeds).  NULL (the default) restores the
 * plain seeds; launches made while nothing is registered are unaffected, bit for bit.  Process-wide. */
int clipk_set_dropout_epoch(const uint32_t* epoch_dev);

/* ------------------------------------------------------------------------------------------------
 * Token embedding (ESM-2): x[t,:] = table[ids[t],:] * scale[b] * mask[t], with the token-dropout
 * rescale (modeling_esm.py:252-268) folded into row_scale[B] by the caller.  f32 out.
 */
int clipk_embed_fwd(const int64_t* ids, const float* table, const float* row_scale /*[B] or NULL*/,
                    const uint8_t* mask /*[B*L] or NULL*/, int mask_token_id,
                    float* x, int B, int L, int d, int V /* table rows: ids outside [0, V) give NaN rows */, void* stream);
/* dtable[V,d] += sum over tokens (torch embedding backward).  V <= 64 (ESM-2: 33): one-hot product on the exact-f32
 * matrix pipe with fixed-order reductions, bitwise reproducible, needs the workspace below; larger vocabularies (or
 * workspace == NULL): per-block LDS tables + float atomics. */
size_t clipk_embed_bwd_workspace(int B, int L, int d, int V);
int clipk_embed_bwd(const int64_t* ids, const float* dx, const float* row_scale, const uint8_t* mask,
                    int mask_token_id, float* dtable, int B, int L, int d, int V,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Pooling over the sequence: mode 0 = position 0 (rna_clip_codes.ipynb:1948), 1 = masked mean
 * (configuration_hybrid_clip.py:109 use_mean_pooling).  x f32 [B,L,d] -> y f32 [B,d].  Any B (sequences beyond grid
 * y's 65 535 are walked by a loop).  The backwards write float4 rows: d % 4 != 0 is CLIPK_ERR_UNSUPPORTED, in
 * clipk_pool_bwd and in clipk_pool_varlen_bwd alike, before anything is launched. */
int clipk_pool_fwd(const float* x, const uint8_t* mask, float* y, int B, int L, int d, int mode, void* stream);
int clipk_pool_bwd(const float* dy, const uint8_t* mask, float* dx, int B, int L, int d, int mode, void* stream);

/* Pooling over packed variable-length batches (sequence b = rows [cu[b], cu[b+1]) of x f32 [T, d]): mode 0 = the first
 * row, 1 = mean over the sequence's rows; an empty sequence (cu[b] == cu[b+1]) gives y[b] = 0 and owns no dx row.  The
 * backward writes rows [cu[0], cu[B]) of dx [T, d] and no other.  cu_seqlens: DEVICE int32 [B+1].  Any B. */
int clipk_pool_varlen_fwd(const float* x, const int* cu_seqlens, float* y, int B, int d, int mode, void* stream);
int clipk_pool_varlen_bwd(const float* dy, const int* cu_seqlens, float* dx, int B, int d, int mode, void* stream);

/* Attention over PACKED variable-length batches.  The reference pads every batch to its longest
 * sequence with NaN rows and masks them as keys (current/rna_clip_codes.ipynb:1824-1857 collate_fn /
 * create_padding_mask, :1936-1946; lengths 30..2542), so padded rows still run through every Linear, LayerNorm and
 * attention row.  Here sequence b is rows [cu_seqlens[b], cu_seqlens[b+1]) of the packed tensors:
 *   qkv bf16 [T, 3*H*D], out / dout bf16 [T, H*D], dqkv bf16 [T, 3*H*D], lse / delta f32 [H, T];
 *   cu_seqlens: DEVICE int32 [B+1] (cu[0] = 0, cu[B] = T); max_len = longest sequence (grid sizing only);
 *   every sequence must have at least one row, cu[b+1] - cu[b] >= 1: a length of 0 is not supported (nor tested);
 *   rope tables (optional, ESM head dims): f32 [>= max_len, D/2], indexed by the position inside the sequence.
 * Arithmetic is that of clipk_attn_fwd / clipk_attn_bwd on each sequence alone. */
int clipk_attn_varlen_fwd(const void* qkv, const int* cu_seqlens, const float* rope_cos, const float* rope_sin,
                          void* out, float* lse, int B, int T, int max_len, int H, int D, float q_scale, float dropout_p,
                          uint32_t dropout_seed, void* stream);
/* clipk_attn_fwd_rot for a packed batch: rotates q / k of every sequence IN PLACE (positions count from the sequence's
 * first row) while the whole-head kernel stages them, for D in {16, 24, 32} and 128 < max_len <= 256 only
 * (CLIPK_ERR_UNSUPPORTED otherwise: use clipk_attn_varlen_fwd, which leaves qkv alone).  Its backward is
 * clipk_attn_varlen_bwd(..., prerotated = 1): one whole-head kernel per (sequence, head) instead of the general pair. */
int clipk_attn_varlen_fwd_rot(void* qkv, const int* cu_seqlens, const float* rope_cos, const float* rope_sin,
                              void* out, float* lse, int B, int T, int max_len, int H, int D, float q_scale, void* stream);
int clipk_attn_varlen_bwd(const void* qkv, const int* cu_seqlens, const float* rope_cos, const float* rope_sin,
                          const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                          int B, int T, int max_len, int H, int D, float q_scale, int prerotated, float dropout_p,
                          uint32_t dropout_seed, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Optimiser step on flat f32 buffers: AdamW (decoupled weight decay, torch.optim.AdamW semantics,
 * rna_clip_codes.ipynb:2033) with the global-norm clip of clip_grad_norm_ (ipynb:2076) folded in:
 *   sumsq kernel -> grad_norm_sq[0] (device), then the update reads it to compute the clip factor.
 * wd_mask: per-element 0/1 float or NULL (all decayed).  Also refreshes the bf16 weight copy.
 */
size_t clipk_sumsq_workspace(int64_t n);
int clipk_sumsq(const float* g, int64_t n, float* out /* device scalar, overwritten */,
                void* workspace, size_t workspace_bytes, void* stream);
/* hyper_dev (optional): DEVICE array {lr, 1 - beta1^t, sqrt(1 - beta2^t)} read by the kernel instead of `lr` / `step` -
 * what changes from step to step lives in memory, so that a whole training step (rna_clip_codes.ipynb:2061-2089) can be
 * captured once in a hipGraph and replayed (clip_dplm_amd.training.GraphedTrainStep); NULL: the scalars. */
int clipk_adamw_step(float* w, const float* g, float* m, float* v, void* w_bf16 /* or NULL */,
                     int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int step, const float* grad_norm_sq /* device scalar or NULL */, float max_norm,
                     float grad_scale, const float* hyper_dev /* or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Entropic optimal transport (Sinkhorn) between two f32 clouds X [Mx,P], Y [Ny,P] with weights a [Mx], b [Ny] (> 0, sum 1)
 * and cost C_ij = |x_i - y_j|^2:   OT_eps = min_P <P,C> + eps KL(P | a (x) b).   The reference's second generation
 * (tong/models/flows/ot_flow.py, SchrodingerBridgeFlow) takes the plan from a library on the materialised matrix; here
 * the M x N matrix is never written.  With S = (2/eps) X Y^T and scaled log-potentials u, v (the squared norms are
 * absorbed into them):
 *     u_i = log a_i - LSE_j(S_ij + v_j),   v_j = log b_j - LSE_i(S_ij + u_i),   start v = log b, one iteration = u then v
 *     plan P_ij = exp(S_ij + u_i + v_j);  duals f_i = eps (u_i - log a_i) + |x_i|^2, g_j = eps (v_j - log b_j) + |y_j|^2
 *     OT_eps = <a,f> + <b,g>;  dOT_eps/dx_i = 2 (r_i x_i - sum_j P_ij y_j), r_i = sum_j P_ij  (envelope theorem)
 *     symmetric problem (X = Y, a = b): u <- (u + log a - LSE(S + u)) / 2, one potential.
 *
 * clipk_sim_lse_bias - one half-iteration:  nv_i = logw[i] - LSE_j(scale[0] <X_i, Y_j> + bias[j])
 *   bias [Ny] or NULL (zeros), logw [Mx] or NULL (zeros), scale: device scalar.  prev [Mx] or NULL: the potential being
 *   replaced; average != 0 (needs prev): out_i = (prev_i + nv_i) / 2, else out_i = nv_i.  err (device scalar or NULL,
 *   needs prev): err[0] += sum_i exp(logw_i) |exp(prev_i - nv_i) - 1|, the L1 distance between the marginal of the plan
 *   with `prev` on this side and its weights.  prev == out is allowed.
 *   Kernel: the tiling of the fused cross-entropy's LSE pass (64 queries per workgroup, 64-key tiles on
 *   v_mfma_f32_32x32x2_f32, a running (max, sum) per lane, keys beyond Ny masked with -inf); key-range splits are merged
 *   in split order by a finalize kernel which also forms the update; the error terms are summed by one workgroup in a
 *   fixed order (a third, tiny launch, only when err is given).  clipk_sim_lse_bias_plan reports the grid: nqb 64-query
 *   blocks x ksplit key splits.
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 768, X / Y / workspace 16-byte aligned.
 * clipk_sinkhorn_apply - plan-weighted sums per row, each output optional (not all NULL):
 *     mass[i] = sum_j P_ij,   bary[i,:] = sum_j P_ij y_j (unnormalised),   cost[i] = sum_j P_ij C_ij
 *   u [Mx], v [Ny]; nx [Mx] = |x_i|^2 and ny [Ny] = |y_j|^2 are read for cost only (C_ij = nx_i + ny_j - 2 <x_i, y_j>).
 *   Kernel: the structure of the fused cross-entropy's gradient pass: S tile, the plan tile into LDS, a second MFMA
 *   product with the staged key rows; key-split slabs are summed in split order.  Without bary the second product and
 *   the slabs are skipped.
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 512, X / Y / bary / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED and the workspace helpers return 0.  Never allocates,
 * never synchronises, capturable, no float atomics: results depend on the shapes alone. */
int clipk_sim_lse_bias_plan(int Mx, int Ny, int* nqb, int* ksplit);
size_t clipk_sim_lse_bias_workspace(int Mx, int Ny, int P);
int clipk_sim_lse_bias(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale /* device scalar */,
                       const float* bias /*[Ny] or NULL*/, const float* logw /*[Mx] or NULL*/,
                       const float* prev /*[Mx] or NULL*/, int average, float* out /*[Mx]*/,
                       float* err /* device scalar, accumulated, or NULL */, void* workspace, size_t workspace_bytes,
                       void* stream);
/* clipk_sim_lse_bias_x3 - the half-iteration of clipk_sim_lse_bias with the product on the bf16 matrix pipe (bf16x3):
 *     nv_i = logw[i] - LSE_j(scale[0] A_ij + bias[j]),   A_ij = sum_p hi(x)hi(y) + hi(x)lo(y) + lo(x)hi(y)   (f32 sums)
 *   Xhi / Xlo [Mx, PP] and Yhi / Ylo [Ny, PP]: the planes clipk_split_bf16 writes (row pitch PP = P rounded up to 32, pads
 *   zero).  Both clouds are queries in one half-iteration and keys in the other: split each once per solve.  bias, logw,
 *   prev, average, out and err (accumulated, fixed-order reduce) as in clipk_sim_lse_bias; prev == out is allowed; scale
 *   is a device scalar; keys beyond Ny are masked with -inf.
 *   Error bound (the "Certificate" of the prefiltered top-k above, same eps_rel and eps_abs): for every pair
 *     |scale A_ij - scale <x_i, y_j>| <= eta_i = |scale| |x_i| max_j|y_j| eps_rel + eps_abs,
 *   eps_rel = the bf16x3 value (retrieval.prefilter_eps_rel(P, "bf16x3")).  LSE is non-expansive in the sup norm, so
 *   |nv_x3 - nv_exact| <= eta = max_i eta_i.  A_ij with x as the query need not equal A_ji with y as the query bit for
 *   bit (the MFMA's summation order is not documented): only the bound is promised, not symmetry.
 *   Kernel: the 128-query x 64-key tile of the prefilter's candidate pass (three v_mfma_f32_32x32x16_bf16 per fragment
 *   pair), the running (max, sum) of clipk_sim_lse_bias as its epilogue, the same finalize and error kernels.
 *   clipk_sim_lse_bias_x3_plan reports the grid: nqb 128-query blocks x ksplit key splits.
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 768, planes / workspace 16-byte aligned; anything else returns
 *   CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED and the workspace helper returns 0.  Never allocates, never synchronises,
 *   capturable, no float atomics: two runs give identical bits.  Non-finite inputs are as undefined as in the f32 entry. */
int clipk_sim_lse_bias_x3_plan(int Mx, int Ny, int* nqb, int* ksplit);
size_t clipk_sim_lse_bias_x3_workspace(int Mx, int Ny, int P);
int clipk_sim_lse_bias_x3(const void* Xhi, const void* Xlo, int Mx, const void* Yhi, const void* Ylo, int Ny, int P,
                          const float* scale /* device scalar */, const float* bias /*[Ny] or NULL*/,
                          const float* logw /*[Mx] or NULL*/, const float* prev /*[Mx] or NULL*/, int average,
                          float* out /*[Mx]*/, float* err /* device scalar, accumulated, or NULL */, void* workspace,
                          size_t workspace_bytes, void* stream);
size_t clipk_sinkhorn_apply_workspace(int Mx, int Ny, int P);
int clipk_sinkhorn_apply(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale /* device scalar */,
                         const float* u /*[Mx]*/, const float* v /*[Ny]*/, const float* nx /*[Mx]*/,
                         const float* ny /*[Ny]*/, float* mass /*[Mx] or NULL*/, float* bary /*[Mx,P] or NULL*/,
                         float* cost /*[Mx] or NULL*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Draws from the entropic plan without the matrix.  The conditional of P_ij = exp(S_ij + u_i + v_j) along row i is
 * softmax_j(S_ij + v_j) (u_i is constant along the row), and the arg max of Gumbel-perturbed logits is a draw from it:
 *
 * clipk_sim_sample - idx[i] = argmax_j z_ij,  z_ij = scale[0] <X_i, Y_j> + bias[j] + G(seed, stream_i, j),  score[i] = max_j z_ij
 *   bias [Ny] or NULL (zeros); score [Mx] or NULL.  seed_offset: two 64-bit integers in device memory, {seed,
 *   stream_offset}; row i of the launch is stream stream_offset + i (64-bit).  They are read by the kernel, so a captured
 *   graph draws fresh noise on every replay once the caller bumps them.
 *   The noise is part of the contract (tests/sinkhorn_sample_ref.py restates it on the CPU):
 *     Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), key = (low, high 32 bits
 *     of seed), counter = (j >> 2, low 32 bits of the stream, high 32 bits of the stream, 0); key j takes output word
 *     j & 3 = w;  U = ((w >> 9) + 0.5) 2^-23, exact in f32 and in [2^-24, 1 - 2^-24];  G = -log(-log U).
 *   A higher z wins and equal z goes to the lower key index, at every level of the merge: the result depends on (inputs,
 *   seed, stream) only, never on the grid - rows [r0, r1) of a launch equal a launch of those rows with stream_offset + r0.
 *   Kernel: the tiling and the key-range split plan of clipk_sim_lse_bias (clipk_sim_lse_bias_plan reports the grid),
 *   a running (best value, best key) per lane in place of (max, sum), keys beyond Ny masked with -inf, one Philox call
 *   per four consecutive keys per query; the key splits are merged in split order by a finalize launch.
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 768, X / Y / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED and the workspace helper returns 0.  Never allocates,
 * never synchronises, capturable, no float atomics. */
size_t clipk_sim_sample_workspace(int Mx, int Ny, int P);
int clipk_sim_sample(const float* X, int Mx, const float* Y, int Ny, int P, const float* scale /* device scalar */,
                     const float* bias /*[Ny] or NULL*/, const long long* seed_offset /* device: {seed, stream_offset} */,
                     long long* idx /*[Mx]*/, float* score /*[Mx] or NULL: the winning z*/, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Row sums over a mixture of Gaussian kernels between two f32 clouds X [Mx,P], Y [Ny,P] without the Mx x Ny matrix: what
 * a multi-bandwidth MMD (clip_dplm_amd.distribution.mmd2; the 'mmd' of the reference's tong/configs/default.yaml:74)
 * and its gradient are made of.
 *
 * clipk_kernel_sums - each output optional (not both NULL):
 *     d2_ij = max(nx[i] + ny[j] - 2 <X_i, Y_j>, 0),   K_ij = sum_b weights[b] exp(-gammas[b] d2_ij)
 *     ksum[i] = sum_j K_ij,   kbary[i,:] = sum_j K_ij Y_j
 *   gammas [B] (> 0) and weights [B] (any sign) are device vectors the kernel reads: a bandwidth derived from the data
 *   costs no host read.  nx [Mx] = |x_i|^2, ny [Ny] = |y_j|^2.
 *   Diagonal rule: diag_offset = -1 skips nothing; diag_offset >= 0: row i skips key j = i + diag_offset - the term
 *   enters neither output (it is dropped, never formed and subtracted, so no trace of the computed d2 of a point with
 *   itself is left); a row whose skipped key lies at or beyond Ny skips nothing.  A cloud with itself: diag_offset = 0.
 *   Gradient: with weights[b] gammas[b] in place of weights[b] (K'), d/dx_i sum_j K_ij = -2 (ksum'[i] x_i - kbary'[i,:]).
 *   Kernel: the structure of clipk_sinkhorn_apply (64 queries per workgroup, 64-key tiles on v_mfma_f32_32x32x2_f32, the
 *   weight tile into LDS, a second MFMA product with the staged key rows); d2 is formed once per element and the B
 *   exponentials applied to it - one tile walk for every bandwidth; the values lie in (0, 1], so there is no running
 *   maximum; keys beyond Ny contribute 0.  Key-split slabs are summed in split order by a finalize launch; without kbary
 *   the second product and the slabs are skipped.  The grid is that of clipk_sim_lse_bias (clipk_sim_lse_bias_plan).
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 512, 1 <= B <= 8, X / Y / kbary / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED and the workspace helper returns 0.  Never allocates,
 * never synchronises, capturable, no float atomics: results depend on the shapes and inputs alone. */
size_t clipk_kernel_sums_workspace(int Mx, int Ny, int P, int B);
int clipk_kernel_sums(const float* X, int Mx, const float* Y, int Ny, int P,
                      const float* gammas /* device [B], > 0 */, const float* weights /* device [B] */, int B,
                      const float* nx /*[Mx] = |x_i|^2*/, const float* ny /*[Ny] = |y_j|^2*/,
                      long long diag_offset /* -1: none; else row i skips key j == i + diag_offset */,
                      float* ksum /*[Mx] or NULL*/, float* kbary /*[Mx,P] or NULL*/,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The exact (non-entropic) coupling of two equal-size f32 clouds X, Y [N,P] under the cost |x_i - y_j|^2 by the auction
 * algorithm (Bertsekas) without the N x N matrix: with uniform weights the optimal plan is a permutation.  The reference
 * selects it with flow_type == 'exact_ot' (tong/models/flows/triple_flow.py:12-17, ot_flow.py:58-68) and takes it from a
 * library that solves the materialised matrix on the host.
 *
 * clipk_sim_top2_bias - the two best keys of every listed query row:
 *     z_rj   = scale[0] <X[row(r)], Y_j> + bias[j]                 row(r) = rows ? rows[r] : r,   r in [0, Mr)
 *     idx[r] = argmax_j z_rj,   best[r] = max_j z_rj,   gap[r] = best[r] - max_{j != idx[r]} z_rj   (+inf when Ny == 1)
 *   bias [Ny] or NULL (zeros).  rows [Mr] int32 or NULL: indices into X's Mx rows, repeats allowed (without rows,
 *   Mr <= Mx).  n_active: a device int32 or NULL (= Mr): only the list positions below min(n_active[0], Mr) are
 *   computed; a query block at or beyond it returns before its first barrier and outputs beyond it are untouched.
 *   idx int32 [Mr]; best, gap f32 [Mr], each may be NULL.
 *   Rule at every merge level (within a lane, lane halves, the two key-waves, key splits in the finalize launch): the
 *   higher z is best, equal z goes to the lower key, the runner-up is the maximum of what is left - an exact tie gives
 *   gap 0.  The merge of (z1, k1, z2) triples is associative and commutative: the result depends on the inputs alone,
 *   never on the grid or on n_active - rows [r0, r1) of a launch equal a launch of those rows.
 *   Kernel: the tiling of clipk_sim_sample (64 queries per workgroup, 64-key tiles on v_mfma_f32_32x32x2_f32, keys beyond
 *   Ny masked; the query row pointers are a gather) with a running (best, arg best, runner-up) per lane.  The key split
 *   is this entry's own, a fixed number of tiles per split whatever the row count (clipk_sim_top2_bias_plan reports the
 *   grid: nqb 64-query blocks x ksplit key splits): one active query block still fills the device.
 *   Supported: Mx, Mr, Ny >= 1, P % 4 == 0, P <= 768, X / Y / workspace 16-byte aligned.
 *
 * clipk_auction_rounds - n_rounds Jacobi bidding rounds on device state, no host read between them:
 *     assigned [N] int32 row -> key or -1;  owner [N] int32 key -> row or -1 (mutually inverse);
 *     bias [N] f32 = -|y_j|^2 - price_j;  eps: device f32 scalar (> 0), in units of the squared distance.
 *   One round: (1) the unassigned rows are compacted into a list in rising row order; (2) clipk_sim_top2_bias over that
 *   list with scale 2 and the device count; (3) each bidder r offers inc = gap + eps to key idx[r]; a key keeps the
 *   largest offer, an equal offer goes to the lower row (a 64-bit integer atomicMax on (bits of inc, complement of the
 *   row): inc >= 0, so its bit pattern is ordered, and integer max does not depend on the order of arrival); (4) every
 *   key with an offer frees its previous owner, takes the winner and sets bias[j] -= inc; if that leaves bias[j]
 *   unchanged (eps below the f32 resolution of the prices) stalled[0] is set to 1 (it is never cleared here).
 *   On return (in stream order) the state is consistent and n_unassigned[0] is the number of unassigned rows after the
 *   last round.  A round with no bidders changes nothing, so trailing rounds are harmless and the state after k rounds
 *   does not depend on how the calls were chunked (n_rounds = 0 only counts).  N <= 65536 (one workgroup compacts).
 *   Supported: 1 <= N <= 65536, P % 4 == 0, P <= 768, X / Y / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED before any launch and the workspace helpers return 0.
 * Never allocates, never synchronises, capturable, no float atomics. */
int clipk_sim_top2_bias_plan(int Mr, int Ny, int* nqb, int* ksplit);
size_t clipk_sim_top2_bias_workspace(int Mr, int Ny, int P);
int clipk_sim_top2_bias(const float* X, int Mx, const int* rows /*[Mr] or NULL*/, int Mr,
                        const int* n_active /* device int32 or NULL */, const float* Y, int Ny, int P,
                        const float* scale /* device scalar */, const float* bias /*[Ny] or NULL*/, int* idx /*[Mr]*/,
                        float* best /*[Mr] or NULL*/, float* gap /*[Mr] or NULL*/, void* workspace,
                        size_t workspace_bytes, void* stream);
size_t clipk_auction_rounds_workspace(int N, int P);
int clipk_auction_rounds(const float* X, const float* Y, int N, int P, float* bias /*[N]*/,
                         const float* eps /* device scalar */, int* assigned /*[N]*/, int* owner /*[N]*/,
                         int* n_unassigned /* device int32 */, int* stalled /* device int32 */, int n_rounds,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * One Lloyd (k-means) iteration over an f32 cloud X [N,P] with centroids C [K,P] without the N x K score matrix:
 * clip_dplm_amd.cluster.kmeans, what the reference's analyze_embedding_alignment (tong/tests/losses/
 * test_contrastive.py:11-16) takes from a host library.
 *
 * clipk_kmeans_step - two modes, chosen by labels_in:
 *     score_ic  = 2 <X_i, C_c> - nc[c]              nc [K] = |C_c|^2, or zeros for the cosine form (arg max <X_i, C_c>)
 *     labels[i] = argmax_c score_ic (equal scores go to the LOWER c),   best[i] = max_c score_ic
 *     sums[c,:] = sum_{i: labels[i] == c} X_i,      counts[c] = #{i: labels[i] == c}   (f32, exact: N <= 2^24)
 *   The squared distance to the nearest centroid is max(|X_i|^2 - best[i], 0).
 *   Fused mode (labels_in == NULL, K <= 64): labels int32 [N] and best f32 [N] are written, and sums / counts follow
 *   those labels - one launch reads each tile of X once for assignment and update.
 *   Labels-given mode (labels_in int32 [N], K <= 65536): sums / counts follow labels_in (an entry outside [0, K) joins
 *   no cluster); C, nc, labels and best are not touched and may be NULL.
 *   Kernel: the structure of clipk_kernel_sums with the roles turned round - the centroids are the 64 queries on the
 *   lanes, the points the keys of the tile walk (64-point tiles on v_mfma_f32_32x32x2_f32); the score tile goes to LDS,
 *   four threads per point row take the arg max, the row is overwritten with its one-hot, and sums^T is the second MFMA
 *   product with the staged point rows; counts are the column sums of the one-hot tile.  Labels-given mode has no first
 *   product and one workgroup column per 64 centroids.  Point-range splits (the plan of clipk_sim_lse_bias for Mx = K,
 *   Ny = N) are summed in split order by a finalize launch, so for K <= 64 the two modes give bit-identical sums.
 *   Supported: 1 <= N <= 2^24, P % 4 == 0, P <= 512, X / C / sums / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED before any launch and the workspace helper returns 0.
 * Never allocates, never synchronises, capturable, no float atomics: results depend on the shapes and inputs alone. */
size_t clipk_kmeans_step_workspace(int N, int K, int P);
int clipk_kmeans_step(const float* X, int N, const float* C /*[K,P] (fused)*/, int K, int P,
                      const float* nc /*[K] (fused)*/, const int* labels_in /*[N] or NULL: fused mode*/,
                      int* labels /*[N] (fused)*/, float* best /*[N] (fused)*/, float* sums /*[K,P]*/,
                      float* counts /*[K]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-label sums of point-to-point distances between two f32 clouds X [Mx,P], Y [Ny,P] without the Mx x Ny matrix: what
 * the silhouette width of a labeling is made of (clip_dplm_amd.cluster.silhouette_samples) - the quality score the
 * reference's hard-coded KMeans(n_clusters=10) lacks, and per label the separation its analyze_embedding_collapse is after.
 *
 * clipk_label_dist_sums:
 *     out[i, g] = sum over { j < Ny : labels[j] == g, j != i + diag_offset } of d_ij        i < Mx, 0 <= g < G
 *     mode 0 (euclidean):    d_ij = sqrt(max(nx[i] + ny[j] - 2 <X_i, Y_j>, 0))
 *     mode 1 (sqeuclidean):  d_ij = max(nx[i] + ny[j] - 2 <X_i, Y_j>, 0)
 *     mode 2 (cosine):       d_ij = max(1 - <X_i, Y_j>, 0)       (the caller passes unit rows; nx, ny are not read, may be NULL)
 *   labels [Ny] int32: an entry outside [0, G) belongs to no column - that is how a caller leaves points out.
 *   nx [Mx] = |x_i|^2, ny [Ny] = |y_j|^2.
 *   Diagonal rule: diag_offset = -1 skips nothing; diag_offset >= 0: row i skips key j = i + diag_offset - the term is
 *   dropped, never formed and subtracted: a computed d2_ii of rounding size would enter the Euclidean sum as its square
 *   root, about 3e-4 |x|.  A row whose skipped key lies at or beyond Ny skips nothing.  Rows [r0, r1) of a cloud against
 *   the whole cloud: diag_offset = r0.
 *   out [Mx, Gp] with the row stride Gp = G rounded up to a multiple of 4; the padding columns are zeros.
 *   Kernel: the structure of clipk_kernel_sums with kbary (64 queries per workgroup, 64-key tiles on
 *   v_mfma_f32_32x32x2_f32, the distance tile into LDS) with the one-hot of the tile's labels in place of the staged key
 *   rows: out^T[g, q] += H^T[g, key] D[key, q] as the second MFMA product; the one-hot is staged in LDS from the labels
 *   and never exists in memory.  G <= 64: the four waves split the 64 keys of the tile and merge in wave order; beyond,
 *   they split the label rows.  The square root is v_sqrt_f32 (1 ulp).  Key-split slabs are summed in split order by a
 *   finalize launch.  The grid is that of clipk_sim_lse_bias (clipk_sim_lse_bias_plan).
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 512, 1 <= G <= 512, X / Y / out / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED before any launch and the workspace helper returns 0.
 * Never allocates, never synchronises, capturable, no float atomics: results depend on the shapes and inputs alone. */
size_t clipk_label_dist_sums_workspace(int Mx, int Ny, int P, int G);
int clipk_label_dist_sums(const float* X, int Mx, const float* Y, int Ny, int P, const int* labels /*[Ny]*/, int G,
                          int mode /* 0 euclidean, 1 sqeuclidean, 2 cosine */,
                          const float* nx /*[Mx] = |x_i|^2*/, const float* ny /*[Ny] = |y_j|^2*/,
                          long long diag_offset /* -1: none; else row i skips key j == i + diag_offset */,
                          float* out /*[Mx, (G + 3) / 4 * 4]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-label Gaussian masses of each point's perplexity-calibrated neighbourhood, without the Mx x Ny affinities or an
 * N x G one-hot: what LISI (local inverse Simpson's index) and the leave-one-out kernel vote are made of
 * (clip_dplm_amd.mixing).  f32 clouds X [Mx,P], Y [Ny,P].
 *
 * clipk_label_kernel_sums:
 *     d_ij  = max(nx[i] + ny[j] - 2 <X_i, Y_j>, 0)      (cosine: the caller passes unit rows scaled by sqrt(1/2): d = 1 - cos)
 *     t_ij  = d_ij - shift[i]                            (shift NULL: zeros)
 *     w_ij  = exp(-beta[i] t_ij)                         beta [Mx] > 0, PER ROW, read by the kernel from device memory
 *     out[i,g]  = sum over { j < Ny : labels[j] == g, j != i + diag_offset } of w_ij       i < Mx, 0 <= g < G
 *     mass[i]   = sum_g out[i,g]      sumsq[i] = sum_g out[i,g]^2      (g ascending: a fixed order)
 *     top[i]    = arg max_g out[i,g]  (equal values: the lower g),      best[i] = that value
 *   Every output is optional, not all NULL.  out [Mx, Gp] with the row stride Gp = G rounded up to a multiple of 4; the
 *   padding columns are zeros.  Without out the Mx x G result is never written: the finalize launch that sums the
 *   key-split slabs in split order also forms mass, sumsq, top and best, one row per thread, from the same summed values -
 *   the four are bit-identical with and without out.
 *   labels [Ny] int32: an entry outside [0, G) belongs to no column, as in clipk_label_dist_sums - that is how a caller
 *   handles more than 512 labels (one walk per 512) or leaves points out.
 *   Diagonal rule (that of clipk_kernel_sums): diag_offset = -1 skips nothing; diag_offset >= 0: row i skips key
 *   j = i + diag_offset - the term is dropped, never formed and subtracted.  Rows [r0, r1) of a cloud against the whole
 *   cloud: diag_offset = r0.
 *   d is formed exactly as clipk_cond_entropy_sums forms it (the same K-loop, the same norm expansion): with shift = dmin
 *   from that entry the nearest neighbour's term is exactly 1 and every t_ij >= 0.  exp(-beta t) = 2^(c t) with
 *   c = -beta log2 e held in two parts, as clipk_kernel_sums: one v_exp_f32 per element, no division.
 *   Kernel: the walk of clipk_label_dist_sums (both forms of the second product) with one more element function; beta_i,
 *   c and shift_i sit in the row's lane registers.  The grid is that of clipk_sim_lse_bias (clipk_sim_lse_bias_plan).
 *   Supported: Mx, Ny >= 1, P % 4 == 0, P <= 512, 1 <= G <= 512, X / Y / out / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED before any launch and the workspace helper returns 0.
 * Never allocates, never synchronises, capturable, no float atomics, no cooperative launch: results depend on the shapes
 * and inputs alone. */
size_t clipk_label_kernel_sums_workspace(int Mx, int Ny, int P, int G);
int clipk_label_kernel_sums(const float* X, int Mx, const float* Y, int Ny, int P, const int* labels /*[Ny]*/, int G,
                            const float* beta /*[Mx]*/, const float* shift /*[Mx] or NULL*/,
                            const float* nx /*[Mx] = |x_i|^2*/, const float* ny /*[Ny] = |y_j|^2*/,
                            long long diag_offset /* -1: none; else row i skips key j == i + diag_offset */,
                            float* out /*[Mx, (G + 3) / 4 * 4] or NULL*/, float* mass /*[Mx] or NULL*/,
                            float* sumsq /*[Mx] or NULL*/, int* top /*[Mx] or NULL*/, float* best /*[Mx] or NULL*/,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact t-SNE of an f32 cloud X [N,P] into a map Y [N,2] without the N x N matrix (clip_dplm_amd.manifold.tsne): what
 * the reference's Visualizer.plot_embeddings (tong/utils/visualization.py) takes from a host library.
 *
 * Definitions (3 <= N, P % 4 == 0, P <= 512):
 *     d_ij    = max(nx[i] + nx[j] - 2 <X_i, X_j>, 0)                       as in clipk_kernel_sums
 *     m_i     = min_{j != i} d_ij
 *     p_{j|i} = exp(-beta_i (d_ij - m_i)) / s0_i,   s0_i = sum_{j != i} exp(-beta_i (d_ij - m_i))
 *               (subtracting m_i changes nothing mathematically; it keeps the nearest neighbour's term at exactly 1,
 *               so no row underflows to an empty sum)
 *     H_i(beta) = log s0_i + beta s1_i / s0_i,  s1_i = sum_{j != i} (d_ij - m_i) exp(-beta (d_ij - m_i))      (nats)
 *     beta_i solves H_i(beta_i) = log(perplexity)
 *     P_ij    = (p_{j|i} + p_{i|j}) / (2N)
 *     w_ij    = 1 / (1 + |y_i - y_j|^2) for i != j,   Z = sum_{i != j} w_ij
 *     grad_i  = 4 (alpha sum_j P_ij w_ij (y_i - y_j) - (1/Z) sum_j w_ij^2 (y_i - y_j))      alpha: the exaggeration
 *     KL      = sum_{i != j} P_ij (log P_ij - log w_ij) + log Z,   0 log 0 = 0   (no clamp of P or Q at machine epsilon)
 *   Diagonal rule (that of clipk_kernel_sums): the pair (i, i) is dropped as a term, never formed and subtracted.
 *   diag_offset = -1 skips nothing; diag_offset >= 0: row i skips key j = i + diag_offset; a cloud with itself passes 0.
 *
 * clipk_cond_entropy_sums - one walk of X against itself, each output optional (not all NULL):
 *     dmin[i]  = min over the kept keys of d_ij
 *     s0[i,b]  = sum over the kept keys of exp(-betas[i,b] t_ij),   s1[i,b] = sum of t_ij exp(-betas[i,b] t_ij),
 *     t_ij = d_ij - shift[i]       (shift NULL: zeros)
 *   betas [N,B] are PER-ROW candidate bandwidths, 1 <= B <= 8, held in the registers of the row's lane; d is formed once
 *   per element and the B exponentials applied to it.  B = 0 (betas, s0, s1 NULL) asks for dmin alone: the first pass.
 *   With shift = dmin of an earlier call every t_ij >= 0 and the nearest neighbour's term is exactly 1: the same walk
 *   forms the same d bit for bit.  exp(-beta t) = 2^(c t) with c = -beta log2 e held in two parts, as clipk_kernel_sums.
 *   Kernel: the grid, key split and split-order finalize of clipk_kernel_sums without kbary (clipk_sim_lse_bias_plan
 *   reports the grid for Mx = Ny = N).
 *
 * clipk_tsne_grad - one walk per gradient step: rows [N,6] (want_kl) or [N,5], per row i the sums over the kept keys j
 *     rows[i,0:2] = sum_j P_ij w_ij (y_i - y_j)        rows[i,2:4] = sum_j w_ij^2 (y_i - y_j)
 *     rows[i,4]   = sum_j w_ij                          rows[i,5]   = sum_j P_ij (log P_ij - log w_ij)
 *   beta, dmin (= m), log_s0 [N] come from clipk_cond_entropy_sums (log_s0 = log s0 at beta with shift = dmin); Y [N,2].
 *   The entry packs one 32-byte record per point (norm, c in two parts, m, log2 s0, y0, y1) into the workspace; the walk
 *   stages the tile's 64 key records in LDS.  The exponent is -beta (d - m) - log s0 computed from (d - m), never as
 *   a d + b with beta m folded into b.  Per element: two v_exp_f32, one v_rcp_f32, no division; one v_log_f32 more with
 *   want_kl.  The other five sums are bit-identical with and without want_kl.
 *
 * clipk_tsne_update - the reductions of rows in a fixed order (one workgroup) and the delta-bar-delta step:
 *     z[0] = Z = sum_i rows[i,4];  kl[0] = sum_i rows[i,5] + log Z (ncomp = 6 only);  gnorm[0] = |grad|_2
 *     grad = 4 (alpha rows[:,0:2] - rows[:,2:4] / Z)
 *     inc = update * grad < 0;  gains = max(inc ? gains + 0.2 : gains * 0.8, 0.01)
 *     update = momentum * update - lr * gains * grad;   Y += update
 *   z is required and is read back from device memory by the step; kl, gnorm may be NULL.  Y, update, gains [N,2]: all
 *   three, or all NULL for the reductions alone.
 *
 *   Supported: 3 <= N, P % 4 == 0, P <= 512, 0 <= B <= 8, X / workspace 16-byte aligned.
 * Anything else returns CLIPK_ERR_BAD_ARG or CLIPK_ERR_UNSUPPORTED before any launch and the workspace helpers return 0.
 * Never allocates, never synchronises, no host read, capturable, no float atomics, no cooperative launch: results depend
 * on the shapes and inputs alone. */
size_t clipk_cond_entropy_sums_workspace(int N, int P, int B);
int clipk_cond_entropy_sums(const float* X, int N, int P, const float* nx /*[N] = |x_i|^2*/,
                            const float* betas /*[N,B] or NULL (B = 0)*/, int B, const float* shift /*[N] or NULL*/,
                            long long diag_offset /* -1: none; else row i skips key j == i + diag_offset */,
                            float* dmin /*[N] or NULL*/, float* s0 /*[N,B] or NULL*/, float* s1 /*[N,B] or NULL*/,
                            void* workspace, size_t workspace_bytes, void* stream);
size_t clipk_tsne_grad_workspace(int N, int P, int want_kl);
int clipk_tsne_grad(const float* X, int N, int P, const float* nx /*[N]*/, const float* beta /*[N]*/,
                    const float* dmin /*[N]*/, const float* log_s0 /*[N]*/, const float* Y /*[N,2]*/,
                    long long diag_offset, int want_kl, float* rows /*[N, want_kl ? 6 : 5]*/, void* workspace,
                    size_t workspace_bytes, void* stream);
int clipk_tsne_update(const float* rows /*[N,ncomp]*/, int N, int ncomp /* 5 or 6 */, float alpha, float momentum,
                      float lr, float* Y /*[N,2] or NULL*/, float* update /*[N,2]*/, float* gains /*[N,2]*/,
                      float* z /* device scalar */, float* kl /* device scalar or NULL */,
                      float* gnorm /* device scalar or NULL */, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Exact k-nearest-neighbour graph of f32 clouds without the Mx x Ny matrix (clip_dplm_amd.neighbors.knn_graph): the
 * neighbours that kBET and the published (kNN-truncated) LISI are made of - the batch-mixing scores the metric list
 * of the reference's tong/experiments/evaluate.py (:39-47, compute_all_metrics / BiologicalMetrics) lacks, and the
 * local view beside the KMeans + ARI of its analyze_embedding_alignment (tong/tests/losses/test_contrastive.py:11-16).
 *
 * clipk_sim_knn: the walk, register lists and merge tree of clipk_sim_topk with three additions:
 *     z_ij = fl(fl(scale * s_ij) + bias[j])      s_ij: the accumulator bits of clipk_sim_topk; two separate roundings (no
 *                                                fma); bias [Ny] device f32, NULL: the add is skipped
 *     eligible(i, j):  j != i + diag_offset                                   (diag_offset = -1: no key skipped)
 *                 and  (after_s == NULL  or  z_ij < after_s[i]  or  (z_ij == after_s[i] and j > after_i[i]))
 *     scores[i, 0..k) / idx[i, 0..k) = the k best eligible (z_ij, j) of row i in the order of clipk_sim_topk (z descending,
 *     equal z by the lower j), 1 <= k <= 64; with fewer than k eligible keys the trailing slots are (-inf, -1).
 *   (after_s, after_i) [Mx] (both or neither) is a CURSOR: a position in the total order, after which the row resumes.  Fed
 *   the last column of the previous call it returns the next k keys, so k is not bound by the 64 list registers.  It holds
 *   the index as well as the score because a run of keys with equal z may straddle the boundary between two calls: a
 *   score threshold alone would return the rest of the run twice (<=) or never (<).  A cursor (-inf, -1) - the tail of a
 *   short list - leaves no key eligible.
 *   Euclidean neighbours: scale = 1, bias[j] = -|Y_j|^2 / 2; z descending is |X_i - Y_j|^2 = |X_i|^2 - 2 z ascending.
 *   With bias, cursor and diag_offset absent the results are the bits of clipk_sim_topk.
 *   An ineligible key counts as -inf in the per-tile maximum test, so the common path stays one max and one compare per
 *   tile.  A tile's 64 biases reach the lanes through LDS, loaded one tile ahead.  List sizes 1 / 8 / 16 / 64 (the 32-slot
 *   instance measured slower than the 64-slot one at large shapes; results do not depend on the list size).  Contract of clipk_sim_topk: finite inputs, P % 4 == 0, X / Y 16-byte aligned, results bitwise independent of
 *   the split plan (option retrieval_splits), never allocates, never synchronises, capturable, no float atomics; bad
 *   shapes return CLIPK_ERR_* before any launch and the workspace helper returns 0.
 *
 * clipk_pair_sqdist: d2[i, t] = sum_p (X[i,p] - Y[idx[i,t], p])^2 in f32 from the differences (|x|^2 + |y|^2 - 2 <x, y>
 *   cancels exactly where neighbours are closest).  Order: four running sums over the columns p = c mod 4, ascending p,
 *   a_c = fma(d, d, a_c) with d = fl(x - y); d2 = fl(fl(a_0 + a_1) + fl(a_2 + a_3)).  |d2 - exact| <= (P / 4 + 5) 2^-24
 *   exact (to first order).  An index outside [0, Ny) gives +inf.  The graph's order is that of z; these are the accurate distances of
 *   those pairs and may therefore be out of order by rounding-sized amounts.  P % 4 == 0, X / Y 16-byte aligned. */
size_t clipk_sim_knn_workspace(int Mx, int Ny, int P, int k);
int clipk_sim_knn(const float* X, int Mx, const float* Y, int Ny, int P, float scale, const float* bias /*[Ny] or NULL*/,
                  long long diag_offset, const float* after_s /*[Mx] or NULL*/, const int64_t* after_i /*[Mx] or NULL*/,
                  int k, float* scores /*[Mx,k]*/, int64_t* idx /*[Mx,k]*/, void* workspace, size_t workspace_bytes,
                  void* stream);
int clipk_pair_sqdist(const float* X, int Mx, const float* Y, int Ny, int P, const int64_t* idx /*[Mx,k]*/, int k,
                      float* d2 /*[Mx,k]*/, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sparse symmetric operator on a block of f64 vectors (clip_dplm_amd.diffusion: the diffusion map's T = S W S, never
 * materialised; the reference gets X_diffmap / dpt_pseudotime from scanpy on the host - run1/full.py:108,
 * tong/utils/data.py:27-54).  One entry serves the plain operator, a Chebyshev three-term step
 * Y = a (T X - c X) - b X_prev (alpha = a, B = X, beta = -a c, C = X_prev, gamma = -b) and a Lanczos step.
 *
 *   Y[i, c] = alpha * s_i * sum_{e in row i} (w_e * s_{col_e}) * X[col_e, c]  +  beta * B[i, c]  +  gamma * C[i, c]
 *
 * CSR: indptr int64 [N + 1] (indptr[0] = 0, ascending, indptr[N] = nnz), indices int32 [nnz], w f64 [nnz]; s f64 [N] or
 * NULL (all ones); X, B, C, Y f64 [N, m] row-major, 1 <= m <= CLIPK_SPMM_MAX_M (else CLIPK_ERR_UNSUPPORTED); B and C may
 * be NULL.  Y may be B or C (each element is read before it is written, by the same lane); Y may not overlap X
 * (CLIPK_ERR_BAD_ARG).  workspace: clipk_csr_spmm_workspace(nnz, m) bytes (0 for nnz <= CLIPK_SPMM_CHUNK).
 *
 * THE ARITHMETIC (f64, every operation rounded once, to nearest; no fma; independent of the launch shape, of the
 * alignment of the operands and of the device's occupancy - a numpy restatement reproduces every bit):
 *   coef_e = s ? fl(w_e * s[col_e]) : w_e
 *   row i's entries e = indptr[i] .. indptr[i + 1] - 1 are cut into chunks of CLIPK_SPMM_CHUNK, counted from the row's start;
 *   chunk sum   p_q = (((+0 + fl(coef_e X[col_e, c])) + fl(coef_e' X[col_e', c])) + ...)   in ascending e
 *   row sum     t   = ((p_0 + p_1) + p_2) + ...                  in chunk order; an empty row has t = +0
 *   r = s ? fl(s_i * t) : t;   y = fl(alpha * r);   B: y = fl(y + fl(beta * B[i, c]));   C: y = fl(y + fl(gamma * C[i, c]))
 *   (a NULL B or C is skipped, not multiplied by zero; alpha = 0 still multiplies: a non-finite r stays non-finite).
 *   An entry whose column lies outside [0, N) is skipped.  Repeated columns and zero weights are ordinary entries.
 * A group of lanes owns a (row, chunk); chunks q >= 1 are summed by a first launch into the workspace and added by the
 * row's group: a hub row costs its group one chunk plus one partial per further chunk.  No float atomics; never
 * allocates, never synchronises, capturable. */
#define CLIPK_SPMM_CHUNK 64
#define CLIPK_SPMM_MAX_M 64
size_t clipk_csr_spmm_workspace(long long nnz, int m);
int clipk_csr_spmm_f64(const int64_t* indptr /*[N+1]*/, const int32_t* indices /*[nnz]*/, const double* w /*[nnz]*/,
                       const double* s /*[N] or NULL*/, int N, long long nnz, int m, const double* X /*[N,m]*/,
                       double alpha, const double* B /*[N,m] or NULL*/, double beta, const double* C /*[N,m] or NULL*/,
                       double gamma, double* Y /*[N,m]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edges of a kNN graph counted by (label of the row, label of the neighbour): the G x G table that PAGA's cluster graph
 * (clip_dplm_amd.paga; the reference runs sc.tl.paga on the host before its diffusion map - tong/utils/data.py:47) and
 * a kNN label-transfer confusion matrix are made of, in one pass over the [M, k] indices, with no intermediate that
 * grows with M x G.
 *
 *   counts[a, b] += #{(i, t) : row_labels[i] = a, 0 <= idx[i, t] < Ny, key_labels[idx[i, t]] = b}     a, b in [0, G)
 *
 * idx int64 [M, k] (clipk_sim_knn's output; a graph of a cloud against itself has key_labels = row_labels, Ny = M);
 * row_labels int32 [M], key_labels int32 [Ny]; counts int64 [G, G] row-major is ADDED into: the caller zeroes it.
 * A row label outside [0, G), an index outside [0, Ny) (the -1 of a missing result) and a key label outside [0, G)
 * each count nowhere.  M >= 1, Ny >= 1, 1 <= k <= 1024 (else CLIPK_ERR_BAD_ARG), 1 <= G <= CLIPK_LABEL_PAIRS_MAX_G
 * (G < 1: CLIPK_ERR_BAD_ARG, larger: CLIPK_ERR_UNSUPPORTED; the table is at most 8 MB).  Pointers need only their
 * types' alignment.
 * Integer arithmetic: the result is exact and does not depend on the launch shape, on the order of the atomics or on
 * which path ran.  G <= 128: every workgroup keeps the table as int32 bins in LDS, walks a contiguous range of rows
 * (fewer than 2^31 entries, so no bin overflows) and adds its non-zero bins to counts once, with 64-bit atomics.
 * Larger G: a wave merges the equal (a, b) among its lanes and adds once per distinct pair.  No workspace, no host
 * read, never allocates, never synchronises, capturable. */
#define CLIPK_LABEL_PAIRS_MAX_G 1024
int clipk_knn_label_pairs(const int64_t* idx /*[M,k]*/, long long M, int k, const int32_t* row_labels /*[M]*/,
                          const int32_t* key_labels /*[Ny]*/, long long Ny, int G, long long* counts /*[G,G]*/,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CLIPK_H */
