// Host-side launchers of the gfx950 kernels.  Every launcher validates operand shapes on the host
// before the launch (a faulting kernel can reset the whole node) and returns MUDPT_OK / error code.
#pragma once
#include "common.h"

namespace mudpt {

// ------------------------------------------------------------------------------------------------
// MFMA GEMM  C[M,N] = A[M,K] . B[N,K]^T  (both operands K-contiguous, dtype bf16 or fp16,
// fp32 accumulate) with a fused epilogue.  nn.Linear stores weight [out,in] = B; the dX GEMMs of
// the frozen layers use a pre-transposed copy of the weight, so one layout serves fwd and bwd.
// ------------------------------------------------------------------------------------------------
enum Epilogue : int {
    EPI_STORE = 0,     // out0 (T)   = acc + bias
    EPI_GELU = 1,      // out0 (T)   = u = acc + bias ; out1 (T) = QuickGELU(u)
    EPI_RESIDUAL = 2,  // out0 (f32) = aux (f32) + acc + bias
    EPI_GELU_BWD = 3,  // out0 (T)   = acc * QuickGELU'(aux (T))
    EPI_PATCH = 4,     // out0 (f32) [(m / P) * L + 1 + m % P] = acc + pos[1 + m % P]   (patch embed)
    EPI_STORE_F32 = 5  // out0 (f32) = acc + bias
};

struct GemmArgs {
    const void* A = nullptr;  // [M, K], row stride lda (elements)
    const void* B = nullptr;  // [N, K], row stride ldb
    int M = 0, N = 0, K = 0, lda = 0, ldb = 0;
    const float* bias = nullptr;  // [N] or null
    void* out0 = nullptr; int ldo0 = 0;
    void* out1 = nullptr; int ldo1 = 0;
    void* out1_lo = nullptr;       // EPI_GELU only: the low half of out1 as a split operand (common.h LoMode; same row stride in bytes as out1)
    int out1_lo_mode = LO_F16;     // ... its form: LO_F16 (T) or LO_F8 (e4m3 bytes)
    // Split A operand (common.h): a second pass contracts the low half A_lo (same row stride in bytes as A) against B (lo_mode LO_F16)
    // or against the e4m3 weights B8 (LO_F8: [N, K] bytes at the row stride of B in bytes, block scale 2^(b8_scale - 127)); K % 128 == 0 then.
    const void* A_lo = nullptr; int lo_mode = LO_NONE;
    const void* B8 = nullptr; int b8_scale = 127;
    const void* aux = nullptr; int ldaux = 0;
    // QuickGELU' in 8 bits (common.h): EPI_GELU stores out0 = byte codes of QuickGELU'(u) (row stride ldo0 BYTES) instead of u in T;
    // EPI_GELU_BWD reads such codes from aux (row stride ldaux BYTES) instead of u
    bool gelu_q8 = false;
    int flags = 0;                 // bit 0: no XCD remap of the block id (tuning)
    int patches = 0, seq_len = 0;  // EPI_PATCH: P, L
    const float* pos = nullptr;    // EPI_PATCH: [1 + P, N]
    // split K (gemm_nt_kernel, EPI_STORE_F32 partials): slice z = blockIdx.y contracts k in [z * ksplit, (z + 1) * ksplit) and writes its
    // fp32 partial tile set to out0 + z * split_stride elements; launch_gemm sums the slices in order afterwards (splitk_reduce_kernel)
    int ksplit = 0; size_t split_stride = 0;
};
// Host-side options of one launch (never passed to the device): they belong to the calling model handle, not to the process.
struct GemmOpts {
    int variant = 0;                                 // tuning knob, see gemm.hip (mudpt_model_set "gemm_variant")
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;  // if set, a gemm_pp_kernel launch records them (start / end of the kernel)
    // fp32 scratch of the calling stream (one per tower: the towers run concurrently) for split-K partials; null = never split
    float* scratch = nullptr; size_t scratch_elems = 0;
};
int launch_gemm(int dtype, int epi, const GemmArgs& a, hipStream_t s, const GemmOpts& o = GemmOpts());
bool gemm_uses_pp(int epi, const GemmArgs& a, int variant = 0);  // true if launch_gemm dispatches to gemm_pp_kernel
// Which kernel runs a launch: EVERY threshold and knob value is decided here, in host arithmetic with no HIP call (reads a.M, a.N, a.K,
// a.ldo0, a.ldo1, a.ldaux, a.lo_mode; o.variant, o.scratch, o.scratch_elems; ncu = the device's compute units).  launch_gemm switches on the
// result; include/mudpt.h (MUDPT_GEMM_*) names the kernel behind each form.  slices > 1 only for the two split-K forms.
enum GemmForm : int {
    GEMM_PP = MUDPT_GEMM_PP, GEMM_T256x256 = MUDPT_GEMM_T256x256, GEMM_T128x256 = MUDPT_GEMM_T128x256, GEMM_T256x128 = MUDPT_GEMM_T256x128,
    GEMM_T64x64_K128 = MUDPT_GEMM_T64x64_K128, GEMM_T64x64 = MUDPT_GEMM_T64x64, GEMM_T128x64_RING4 = MUDPT_GEMM_T128x64_RING4,
    GEMM_T128x128 = MUDPT_GEMM_T128x128, GEMM_SPLITK_K128 = MUDPT_GEMM_SPLITK_K128, GEMM_SPLITK_K64 = MUDPT_GEMM_SPLITK_K64
};
struct GemmPlan { GemmForm form; int slices; };
GemmPlan gemm_form(int epi, const GemmArgs& a, const GemmOpts& o, int ncu);
// the checks of launch_gemm that read no pointer (shape, strides, epilogue and split-operand codes): what mudpt_gemm_form can refuse
bool gemm_shape_ok(int epi, const GemmArgs& a);
int launch_gemm_pp(int dtype, int epi, const GemmArgs& a, hipStream_t s, const GemmOpts& o);  // persistent 256x256 ping-pong kernel (gemm_pp.hip)

// ------------------------------------------------------------------------------------------------
// LayerNorm over the last dim (fp32 statistics, eps 1e-5; clip/model.py:164-170).
// rows = number of normalised rows; row r reads x[row_index ? row_index[r] : r].
// ------------------------------------------------------------------------------------------------
struct LnFwdArgs {
    const float* x = nullptr; int ldx = 0;     // fp32 input rows
    const int* row_index = nullptr;            // optional gather of input rows
    const float* gamma = nullptr; const float* beta = nullptr;
    void* out = nullptr; int ldo = 0;          // T or fp32 (out_f32)
    void* out_lo = nullptr;                    // optional (T only): y - out, the low half of a split operand (row stride of out in bytes)
    int lo_mode = LO_F16;                      // ... its form (common.h LoMode)
    float* mean = nullptr; float* rstd = nullptr;  // [rows] saved statistics (may be null)
    int rows = 0, d = 0; bool out_f32 = false;
    // Fused residual add + prompt splice (identity row map only): v = x[r] + add[r]; rows (r % ov_L) in
    // [ov_row0, ov_row0 + ov_n) are REPLACED by ov_rows[(r % ov_L) - ov_row0] (the deep-prompt splice,
    // clip/model.py:281-297); v is written to xout[r] (the block input the backward needs) and normalised.
    const float* add = nullptr; int ldadd = 0;
    const void* add_lp = nullptr;              // ... or the addend in T (stride ldadd) when the update stream is kept in T
    float* xout = nullptr; int ldxout = 0;
    const float* ov_rows = nullptr; int ov_row0 = 0, ov_n = 0, ov_L = 1;
};
int launch_ln_fwd(int dtype, const LnFwdArgs& a, hipStream_t s, const LaunchProf* prof = nullptr);

struct LnBwdArgs {
    const void* dy = nullptr; int lddy = 0; bool dy_f32 = false;  // grad of LN output (T or fp32), compact rows
    const float* x = nullptr; int ldx = 0;    // LN input rows (gathered through row_index like fwd)
    const int* row_index = nullptr;
    const float* mean = nullptr; const float* rstd = nullptr; const float* gamma = nullptr;
    const float* dres = nullptr; int lddres = 0;  // optional residual gradient added to the result (same row map as out)
    const void* dres_lp = nullptr;                // ... or the same in T (stride lddres) when the gradient stream is kept in T
    float* dx = nullptr; int lddx = 0;        // fp32 result rows, written at row_index[r] (scatter) or r; may be null if dx_lp is set
    void* dx_lp = nullptr; int lddx_lp = 0;   // optional T copy of the result
    int rows = 0, d = 0;
    bool by_token = false;  // dy / mean / rstd rows are indexed by the token row (row_index[r]) instead of r
    bool stats_by_token = false;  // only mean / rstd are indexed by the token row; dy stays compact (row r)
    // Backward of the prompt splice, fused (identity row map only): result rows whose position inside their sequence (r % side_L) lies in
    // [side_row0, side_row0 + side_n) go, in fp32, to side[(r / side_L) * side_ldb + (pos - side_row0) * d] instead -- the gradient of
    // the spliced-in prompt row -- and ZERO is written to dx / dx_lp: the rows the splice overwrote receive no gradient (clip/model.py:281-297).
    float* side = nullptr; int side_row0 = 0, side_n = 0, side_L = 1; size_t side_ldb = 0;
};
int launch_ln_bwd(int dtype, const LnBwdArgs& a, hipStream_t s, const LaunchProf* prof = nullptr);

// ------------------------------------------------------------------------------------------------
// Attention on packed qkv [B, L, 3*H*64] (q | k | v, heads contiguous inside each third), head dim 64.
// Sequences are independent, on one condition: ROWS OF ANOTHER SEQUENCE MUST BE FINITE.  The kernels work on rows padded to Lp = 32 * ceil(L / 32)
// and several of them load whole padded images (LDS-DMA): image rows L .. Lp - 1 of sequence b are the first rows of sequence b + 1 in
// qkv and dout (zeros past the end of the tensor: the loads are bounds-checked against B * L rows, nothing beyond the tensors is read).
// Those rows only ever meet P = 0 (padded keys start their scores at -inf, padded queries carry lse = -inf), and 0 x finite adds an exact
// zero: a sequence's out, lse, dqkv and delta do not depend on its neighbours' VALUES -- but an Inf / NaN row would poison the sequence
// before it (masking K and V instead would cost the hot path).  Nothing is written outside [B, L] rows of out / dqkv and [B, H, Lp] of
// lse / delta; the forward leaves lse[.., L:Lp] = 0.  tests/test_attention_forms_gpu.py holds every instantiation to this.
// ------------------------------------------------------------------------------------------------
struct AttnArgs {
    const void* qkv = nullptr;  // T [B, L, 3*H*64]
    void* out = nullptr;        // fwd: T [B, L, H*64] (row stride ld_out elements, 0 = H*64)
    void* out_lo = nullptr;     // fwd, optional: out_lo = O - out, the low half of a split operand (same row stride in bytes)
    int lo_mode = LO_F16;       // ... its form (common.h LoMode)
    int ld_out = 0;
    float* lse = nullptr;       // [B, H, Lp] natural-log-sum-exp of the scaled scores (Lp = padded L)
    const void* dout = nullptr; // bwd: T [B, L, H*64]
    void* dqkv = nullptr;       // bwd: T [B, L, 3*H*64]
    float* delta = nullptr;     // bwd scratch [B, H, Lp]
    // bwd, optional: dout is zero except on ONE row per sequence, token row sel_rows[b] (the last block: only the CLS / EOT row of its
    // output is used): dQ is computed for that row's 16-query block only (zero elsewhere) and dK / dV sum over that block's chunk
    const int* sel_rows = nullptr;
    // bwd, optional: only the dqkv rows win_row0 .. win_row0 + win_n - 1 of every sequence are wanted (block 0 of a tower: its input
    // gradient is needed on the prompt rows only).  The 16-row blocks that hold such a row are computed in full -- dQ from all keys,
    // dK / dV from all queries, same sums in the same order as without the window -- and every other row of dqkv is left UNWRITTEN.
    // A window selects the two-kernel / staged form (attn_form), whose kernels honour it.
    int win_row0 = 0, win_n = 0;
    int B = 0, L = 0, H = 0; bool causal = false;
    // exact-fp32 forward (attention_exact.hip): q | k | v in fp32 [B, L, 3*H*64] and, optionally, where to leave their T copy for the backward
    const float* qkv32 = nullptr;
    void* qkv_lp = nullptr;
};
// Single-query forms for the last block (attention_single.hip): ONE query row per sequence (token row a.sel_rows[b]) against all keys
// (causal: the first pos + 1).  q_sel / dout_sel / dq_sel are compact [B, H*64]; out_sel has row stride ld_out (optional low half out_lo);
// the backward writes the k and v thirds of a.dqkv for EVERY row (zeros behind a causal limit) and leaves its q third untouched.
int launch_attn_fwd_single(int dtype, const AttnArgs& a, const void* q_sel, void* out_sel, void* out_lo, int ld_out, float* lse_sel, hipStream_t s);  // out_lo in a.lo_mode
int launch_attn_bwd_single(int dtype, const AttnArgs& a, const void* q_sel, const void* out_sel, int ld_out, const void* dout_sel, const float* lse_sel,
                           void* dq_sel, hipStream_t s);
int attn_padded_len(int L);
// Host-side options of one launch (never passed to the device), as GemmOpts: the A/B switches of the model's knobs and of the test exports
struct AttnOpts {
    bool tiled_fwd_16 = false;  // fwd, 224 < L <= 640: the staged 16-query-block kernel instead of the resident form
    bool two_kernels = false;   // bwd: the dQ kernel + dK/dV kernel pair (L > 224: the staged pair) instead of the default form
    bool force_fused = false;   // bwd, L <= 224: the fused single pass also where the default is another form
    bool fused_w1 = false;      // bwd, fused form: NC waves with two 16-row blocks each instead of 2 NC waves with one
    bool sweep = false;         // bwd, L <= 96, non-causal: the single-sweep kernel (the default only from L = 97 on)
    const LaunchProf* prof = nullptr;  // events around the launch (both kernels of a two-kernel form)
};
// Which kernels run a launch: EVERY threshold and switch is decided here, in host arithmetic with no HIP call (1 <= a.L <= 4096; reads
// a.L, a.causal, a.sel_rows, a.win_n).  The launchers switch on the result; attention.hip's header lists the kernels behind each form.
enum AttnForm : int {
    FWD_PAIR = MUDPT_ATTN_FWD_PAIR, FWD_PERSISTENT = MUDPT_ATTN_FWD_PERSISTENT, FWD_RESIDENT = MUDPT_ATTN_FWD_RESIDENT,
    FWD_STAGED = MUDPT_ATTN_FWD_STAGED, BWD_TWO = MUDPT_ATTN_BWD_TWO, BWD_FUSED_W2 = MUDPT_ATTN_BWD_FUSED_W2,
    BWD_FUSED_W1 = MUDPT_ATTN_BWD_FUSED_W1, BWD_SWEEP = MUDPT_ATTN_BWD_SWEEP, BWD_RESIDENT = MUDPT_ATTN_BWD_RESIDENT,
    BWD_STAGED = MUDPT_ATTN_BWD_STAGED
};
AttnForm attn_form(const AttnArgs& a, const AttnOpts& o, bool bwd);
int launch_attn_fwd(int dtype, const AttnArgs& a, hipStream_t s, const AttnOpts& o = AttnOpts());
int launch_attn_bwd(int dtype, const AttnArgs& a, hipStream_t s, const AttnOpts& o = AttnOpts());
// Exact-fp32 forward (the "fp32" mode): reads a.qkv32, writes a.out (fp16 hi) + a.out_lo (fp16 lo, optional) + a.lse and, if a.qkv_lp
// is set, the fp16 copy of q, k, v that the backward kernels read.
int launch_attn_fwd_exact(const AttnArgs& a, hipStream_t s, const LaunchProf* prof = nullptr);
// attention_resident.hip: both streamed operands of a (sequence, head) pair resident in LDS; only where attn_form says FWD_ / BWD_RESIDENT
int launch_attn_fwd_resident(int dtype, const AttnArgs& a, hipStream_t s, const AttnOpts& o);
int launch_attn_bwd_resident(int dtype, const AttnArgs& a, hipStream_t s, const AttnOpts& o);  // dQ (+ delta) kernel, then dK/dV kernel

// ------------------------------------------------------------------------------------------------
// Small / HBM-bound helpers
// ------------------------------------------------------------------------------------------------
// images fp32 [B,3,H,W] -> patches T [B*P, ldk], columns 3*p*p.. zero  (im2col of the stride-p conv, clip/model.py:527-529)
int launch_patchify(int dtype, const float* images, void* patches, int B, int image_size, int patch, int ldk, hipStream_t s);
// the same as a split operand: patches = hi, patches_lo = the remainder in lo_mode (common.h LoMode), both with rows of ldk * 2 bytes
int launch_patchify_split(int dtype, const float* images, void* patches, void* patches_lo, int lo_mode, int B, int image_size, int patch, int ldk, hipStream_t s);
// x[b, row0 + i, :] = rows[i, :] (+ add[i, :])  for i < n : CLS row, prompt rows, deep-prompt splice.
int launch_set_rows(float* x, int B, int L, int d, int row0, int n, const float* rows, const float* add, hipStream_t s);
// dst[r] = src[rows[r]] (gather) / dst[rows[r]] = src[r] (scatter): whole rows of row_bytes (multiple of 16), strides in bytes.
int launch_gather_rows(const void* src, size_t src_stride, const int* rows, void* dst, size_t dst_stride, int nrows, int row_bytes, hipStream_t s);
int launch_scatter_rows(const void* src, size_t src_stride, const int* rows, void* dst, size_t dst_stride, int nrows, int row_bytes, hipStream_t s);
// dst[rows[r], :] += src[r, :] for nrows rows of d elements of T (fp32 add, one rounding); rows must be distinct
int launch_add_rows(int dtype, const void* src, const int* rows, void* dst, int nrows, int d, hipStream_t s);
// out[i, :] = sum_b src[b, row0 + i, :] in fixed order (deterministic); optionally zero the source rows
// (fp32 and its T copy) afterwards: backward of the splice.  accumulate: out += instead of =.
// scale multiplies the sum (undoes the static loss scale of the backward pass).
int launch_reduce_rows(int dtype, float* src, void* src_lp, int B, int L, int d, int row0, int n, float* out,
                       bool zero_src, bool accumulate, float scale, hipStream_t s);
// fp32 C[M,N] = alpha * op(A) . op(B) (+ bias[N]) (+ beta * C); small shapes only (prompt projections, head).
int launch_sgemm(bool transA, bool transB, int M, int N, int K, float alpha, const float* A, int lda,
                 const float* B, int ldb, float beta, float* C, int ldc, const float* bias, hipStream_t s);
// out[n] (+)= sum_m A[m, n]
int launch_colsum(const float* A, int M, int N, int lda, float* out, bool accumulate, hipStream_t s);
// Backward of one trained Linear y = x W^T + b in one launch: dW [out, in] = dy^T x, db [out] = column sums of dy, dx [R, in] = dy W, all dense
// fp32 and WRITTEN; bit-identical to launch_sgemm(tA) + launch_colsum + launch_sgemm on the same operands.  No output may overlap anything.
int launch_linear_bwd(int R, int out, int in, const float* dy, const float* x, const float* W, float* dW, float* db, float* dx, hipStream_t s);
// y = a + b (elementwise fp32)
int launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t s);
// cast fp32 -> T
int launch_cast(int dtype, const float* x, void* y, size_t n, hipStream_t s);
// Cosine-logit head + mean cross-entropy (trainers/mudpt.py:178-182,250), fwd and bwd in one launch each.
struct HeadArgs {
    const float* img = nullptr;   // [B, e] raw image features
    const float* txt = nullptr;   // [C, e] raw text features
    const int64_t* labels = nullptr;  // [B] (bwd / loss only)
    float scale = 1.f;            // exp(logit_scale)
    float* logits = nullptr;      // [B, C]
    float* loss = nullptr;        // [1] mean CE over B (multiplied by loss_weight for the reported value? no: plain mean)
    float* dlogits = nullptr;     // [B, C] scratch
    float* row_loss = nullptr;    // [B] scratch
    float* dimg = nullptr;        // [B, e] grad of raw image features; null in training: none is wanted (a frozen, prompt-free image tower)
    float* dtxt = nullptr;        // [C, e] grad of raw text features
    float* img_n = nullptr;       // [B, e] scratch: normalised features
    float* txt_n = nullptr;       // [C, e]
    float* img_inv = nullptr;     // [B] 1/||img||
    float* txt_inv = nullptr;     // [C]
    float grad_scale = 1.f;       // dlogits = (softmax - onehot) * grad_scale / B  (the caller folds loss scaling in here)
    int B = 0, C = 0, e = 0;
    int B_total = 0;              // every training head, chunked over the images: the batch the mean is taken over (0 = B); then the caller computes the loss (launch_mean)
};
int launch_head_fwd(const HeadArgs& a, hipStream_t s);
int launch_head_bwd(const HeadArgs& a, hipStream_t s);
// Fused form (head.hip): the logit contraction on the matrix cores in exact fp32 (v_mfma_f32_16x16x4_f32), cross-entropy and dlogits
// in the workgroup that made the logit rows.  a.txt == null: keep the normalised text features of the previous call.
bool head_fused_fits(const HeadArgs& a, bool train);
int launch_head_fused_fwd(const HeadArgs& a, hipStream_t s);
int launch_head_fused_train(const HeadArgs& a, hipStream_t s);  // logits + loss + dimg + dtxt (gradients of the raw features; dtxt null, dimg null: skipped)
// The head's backward from a GIVEN logit gradient (the custom-loss step): with the state a head forward left (img_n / img_inv / txt_n / txt_inv),
//   dimg = gmul * (l2norm_bwd(scale * G   . txt_n, img_n, img_inv) + Eimg)   [B, e]      l2norm_bwd(d, n, inv) = inv * (d - n <d, n>) per row
//   dtxt = gmul * (l2norm_bwd(scale * G^T . img_n, txt_n, txt_inv) + Etxt)   [C, e]
// G [B, C] fp32 at row stride ldg >= C, Eimg [B, e], Etxt [C, e]: each may be null (not all three); dimg / dtxt: either may be null (not computed).
// gmul is folded into the scale of the contraction: no pass over G.  G null: no contraction, the outputs are gmul * E (zeros where E is null too).
struct HeadGradArgs {
    const float* img_n = nullptr;    // [B, e]
    const float* img_inv = nullptr;  // [B]
    const float* txt_n = nullptr;    // [C, e]
    const float* txt_inv = nullptr;  // [C]
    const float* G = nullptr;        // [B, ldg]
    const float* Eimg = nullptr;     // [B, e]
    const float* Etxt = nullptr;     // [C, e]
    float* dimg = nullptr;           // [B, e]
    float* dtxt = nullptr;           // [C, e]
    int64_t ldg = 0;
    float scale = 1.f, gmul = 1.f;
    int B = 0, C = 0, e = 0;
};
bool head_grad_fused_fits(const HeadGradArgs& a);  // e % 16 == 0 and e <= 1024: the [16][e] fp32 tile in 64 KB of LDS
bool head_grad_fused(const HeadGradArgs& a);       // the dispatch: it fits, B <= 16 and C <= 16 (head.hip: where the fused form is the faster one)
// form 0: the dispatch; 1: unfused -- launch_sgemm twice + the row-wise normalisation backward (what launch_head_bwd runs behind its
// cross-entropy rows); 2: fused, refused where it does not fit
int launch_head_grad(const HeadGradArgs& a, hipStream_t s, int form = 0);
// CoCoOp (trainers/cocoop.py): per-image text features.  txt / txt_n / txt_inv / dtxt have B * C rows (row i * C + c).
int launch_pair_head_fwd(const HeadArgs& a, hipStream_t s);
int launch_pair_head_bwd(const HeadArgs& a, hipStream_t s);  // loss, dlogits, dtxt (gradient of the raw text features)
int launch_mean(const float* v, int n, float* out, hipStream_t s);  // out[0] = mean(v) in a fixed order
// text-tower input of every (image, class) pair: class prompt + positional embedding, context rows = ctx + meta_net(image) + pos
int launch_cocoop_prompts(float* x0, const float* emb_pos, const float* ctx, const float* bias, const float* pos, int B, int C, int L, int d, int n, hipStream_t s);
// d bias[i] = scale * sum over the classes and the n context rows of the text-input gradient (fp32 dx or its T copy)
int launch_cocoop_dbias(int dtype, const float* dx, const void* dx_lp, float* dbias, int B, int C, int L, int d, int n, float scale, hipStream_t s);
// CoOp (trainers/coop.py, coop.hip): rows / pos [C * n] = token row and prompt position of context row j of class c (caller's class order)
// x[rows[c n + j]] = ctx[csc ? c : 0][j] + tpos[pos[c n + j]]
int launch_coop_splice(float* x, const float* ctx, const float* tpos, const int* rows, const int* pos, int C, int n, int d, bool csc, hipStream_t s);
// shared: dctx[j] = scale * sum_c dx[rows[c n + j]] (fixed order, coop.hip); CSC: dctx[c][j] = scale * dx[rows[c n + j]]  (fp32 dx or its T copy)
int launch_coop_dctx(int dtype, const float* dx, const void* dx_lp, const int* rows, float* dctx, int C, int n, int d, bool csc, float scale, hipStream_t s);
// Zero-shot CLIP (trainers/zsclip.py, zeroshot.hip).  out[r, :] = table[tokens[r], :] + pos[positions[r], :] for `rows` packed token rows of d
// fp32 (d % 4 == 0): token_embedding + positional_embedding of one prompt template from ids (clip/model.py:827), bit-exact.  tokens / positions
// are DEVICE tables the launcher cannot read: an id outside [0, vocab) or a position outside pos reads out of bounds.
int launch_embed_tokens(const float* table, int vocab, const int* tokens, const int* positions, const float* pos, float* out, int rows, int d, hipStream_t s);
// Prompt ensembling (zsclip.py:107-115), one call per template t in ascending order: v = f / |f| per row; acc = v (first) or acc + v; on the
// last call out = normalise(acc / n_templates) (one template: out = v).  f, acc, out [C, e] fp32, three different tables, e % 4 == 0.
int launch_feature_ensemble(const float* f, float* acc, float* out, int C, int e, bool first, bool last, int n_templates, hipStream_t s);
// y = x / ||x|| per row, inv = 1 / ||x||
int launch_l2norm(const float* x, float* y, float* inv, int rows, int e, hipStream_t s);
int launch_relu(float* y, size_t n, hipStream_t s);
int launch_relu_bwd(float* dy, const float* y, size_t n, hipStream_t s);
// Fused SGD (torch.optim.SGD semantics) over the flat bucket.
int launch_sgd(float* p, const float* g, float* buf, size_t n, float lr, float momentum, float weight_decay,
               float dampening, bool nesterov, bool first_step, hipStream_t s);
// The fused optimizer step (optim.hip): torch 2.10's single-tensor Adam / AdamW (amsgrad) and RMSprop (centered, momentum) rules over a flat
// fp32 bucket in ONE launch; MUDPT_OPTIM_SGD goes through launch_sgd with first_step = (step == 1).  The fields are mudpt_optim's
// (include/mudpt.h), hyper-parameters in double: the host derives 1 - beta, lr / (1 - beta1^step), sqrt(1 - beta2^step) in double, as torch's
// Python does, and rounds each to fp32 once.  state[k]: Adam exp_avg, exp_avg_sq, max_exp_avg_sq (amsgrad); RMSprop square_avg,
// momentum_buffer (momentum > 0), grad_avg (centered); SGD momentum_buffer (momentum != 0); a slot the configuration does not use is not read.
// Refused on the host: a null or (but for SGD) misaligned buffer, n < 1, step < 1, eps <= 0, a beta outside [0, 1), a needed state slot that
// is null, any two of the buffers overlapping.
struct OptimArgs {
    int algo = MUDPT_OPTIM_SGD;
    double lr = 0, beta1 = 0.9, beta2 = 0.999, eps = 1e-8, weight_decay = 0, momentum = 0, alpha = 0.99, dampening = 0;
    bool nesterov = false, amsgrad = false, centered = false;
    int64_t step = 0;  // the 1-based count of this update
    float* p = nullptr; const float* g = nullptr; float* state[3] = {nullptr, nullptr, nullptr};
    int64_t n = 0;
};
int launch_optim(const OptimArgs& a, hipStream_t s);
// The input pipeline on the device (augment.hip; the arguments and the operation: include/mudpt.h at mudpt_augment).  images / params are
// DEVICE tables the launcher cannot read (mudpt_augment_check validates a host copy); mean_std_host is read before the launch returns.
int launch_augment(const uint8_t* pixels, const int64_t* images, int n_images, const int32_t* params, int batch, int size, const float* mean_std_host,
                   float* out, hipStream_t s);
// host arithmetic: MUDPT_AUGMENT_TABLE | R << 8 or MUDPT_AUGMENT_DIRECT for one sample's two axes, -1 for lengths < 1
int augment_form(int x_len, int x_out, int y_len, int y_out, int size);

// ------------------------------------------------------------------------------------------------
// CLIP's ModifiedResNet image tower (resnet.hip; clip/model.py:17-161): the memory movers around its GEMMs.  Activations are NHWC in T, one
// pixel = one row of C channels (C % 8 == 0) at a row stride >= C that is a multiple of 8; every pointer 16-byte aligned
// ------------------------------------------------------------------------------------------------
// patch rows of a 3 x 3, pad 1 convolution of stride 1 | 2: dst [B * Ho * Wo, ldk] T, column (ky * 3 + kx) * C + c, Ho = (H - 1) / stride + 1;
// border taps and columns 9 C .. ldk - 1 are WRITTEN as zeros.  planar: src is fp32 [B, 3, H, W] (C = 3, lds unused), rounded to T
int launch_im2col(int dtype, const void* src, bool planar, int B, int H, int W, int C, int lds, int stride, void* dst, int ldk, hipStream_t s);
// out [M, N] T = act(acc + bias + residual): acc fp32 (a GEMM's EPI_STORE_F32 output), bias [N] fp32 or null, residual T or null, the adds and
// the ReLU in fp32, one rounding; N % 8 == 0, ldacc % 4 == 0
int launch_bias_act(int dtype, const float* acc, int ldacc, const float* bias, const void* residual, int ldres, void* out, int ldo, int M, int N, bool relu, hipStream_t s);
// AvgPool2d(k): [B, H, W, C] -> [B, H / k, W / k, C], fp32 sum in window order times 1 / k^2, one rounding
int launch_avgpool2d(int dtype, const void* src, int lds, void* dst, int ldo, int B, int H, int W, int C, int k, hipStream_t s);
// AttentionPool2d's tokens: [B, HW, C] -> [B, HW + 1, C]; row 0 = the fp32 mean over HW (sum in pixel order times 1 / HW), every row + pos
// [HW + 1, C] fp32, one rounding
int launch_attnpool_tokens(int dtype, const void* src, int lds, const float* pos, void* dst, int ldo, int B, int HW, int C, hipStream_t s);
// AttentionPool2d's attention of the pooled query: q [B, H * 64] fp32 (unscaled; the kernel applies 1 / 8), k / v rows b * L + l of H * 64
// fp32 at stride ldkv -> out [B, H * 64] T; one wave per (image, head), fp32 throughout
int launch_attnpool_attend(int dtype, const float* q, int ldq, const float* k, const float* v, int ldkv, void* out, int ldo, int B, int L, int H, hipStream_t s);
// The convolution as one kernel (conv.hip): out [B Ho Wo, N] T = act(conv_k(src, w) + bias + residual), k = 3 (pad 1, stride 1 | 2) or 1 (stride 1);
// src NHWC T (C % 8 == 0, channel stride lds), w [N, ldk] as mudpt_conv_pack writes it (N % 16 == 0), bias fp32 or null, residual T or null; fp32
// accumulate on the MFMA, the adds and the ReLU in fp32, one rounding.  Reads no channel >= C, no weight column >= k k C, nothing outside the image
int launch_conv2d(int dtype, const void* src, int B, int H, int W, int C, int lds, int k, int stride, const void* w, int ldk, const float* bias, const void* residual,
                  int ldres, void* out, int ldo, int N, bool relu, hipStream_t s);
// host arithmetic: the MUDPT_CONV_* tile launch_conv2d runs M pixels x N channels on, -1 for M or N < 1
int conv2d_form(int M, int N);

// ------------------------------------------------------------------------------------------------
// The linear probe (probe.hip; lpclip/linear_probe.py): one evaluation of the multinomial logistic objective in exact fp32 on the matrix cores
// ------------------------------------------------------------------------------------------------
// C [M, N] = A [M, K] . B [N, K]^T (+ bias[N]): both operands k-contiguous, any M, N, K and strides, 128 x 128 x 32 tiles through LDS
int launch_probe_gemm_nt(int M, int N, int K, const float* A, int lda, const float* B, int ldb, const float* bias, float* C, int ldc, hipStream_t s);
// C [M, N] = A [Kd, M]^T . B [Kd, N] (+ beta W), db [M] (may be null) = column sums of A.  The depth Kd is cut into `slices` runs of whole K-steps
// (0: probe_tn_slices' choice for this device), one workgroup per tile and slice writes its partial sums to scratch (slices * (M N + M) floats),
// and a second kernel adds them in ascending order: no atomics, two runs give the same bits.  C must not alias A, B or W.
int launch_probe_gemm_tn(int M, int N, int Kd, const float* A, int lda, const float* B, int ldb, float beta, const float* W, int ldw, float* C, int ldc, float* db,
                         float* scratch, size_t scratch_numel, int slices, hipStream_t s);
// host arithmetic: the slices launch_probe_gemm_tn runs for a wish of `want` (<= 0: two workgroups per compute unit, at least two K-steps per slice); -1: bad sizes
int probe_tn_slices(int M, int N, int Kd, int want, int ncu);
// Z [rows, n_cls] (row stride ldz) in place: logits -> P = (softmax - onehot(labels)) / rows; row_loss [rows] = logsumexp - z[label];
// loss_sum[0] = their sum, added in double in a fixed order.  labels [rows] int32 in [0, n_cls) are TRUSTED.
int launch_probe_rows(float* Z, int ldz, const int* labels, int rows, int n_cls, float* row_loss, double* loss_sum, hipStream_t s);
// pred[r] = lowest index of the maximum of row r (numpy.argmax); labels / count (both or neither): count[0] = rows with pred == label
int launch_probe_argmax(const float* Z, int ldz, int rows, int n_cls, int* pred, const int* labels, int* count, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// The test pass's evaluator (evaluate.hip; Dassl's Classification evaluator): integer counts in one int32 state buffer, laid out
// [total, correct, invalid, reserved] [support: C] [predicted: C] [hit: C] [cmat: C x C, row = label, column = prediction; with_cmat only]
// ------------------------------------------------------------------------------------------------
size_t eval_state_numel(int n_cls, int with_cmat);  // host arithmetic; 0 for n_cls < 1 or a matrix of 2^31 cells or more
int launch_eval_reset(int* state, int n_cls, int with_cmat, hipStream_t s);
// the prediction of a row is torch.max(logits, 1)[1] on the CPU (lowest index of the maximum, the first NaN if there is one) -- NOT
// probe_row_argmax's rule; a label outside [0, n_cls) only counts as invalid; nothing is reset, launches add up.  pred may be null.
int launch_eval_accumulate(const float* logits, int ldz, const int64_t* labels, int rows, int n_cls, int* state, int with_cmat, int* pred, hipStream_t s);
// results [6] (device doubles) = total, correct, invalid, classes with support, macro-F1 and mean per-class accuracy in percent over those classes
int launch_eval_finalize(const int* state, int n_cls, double* results, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// Top-k in the evaluator's order (topk.hip; eval_order.h states the order): ranked predictions with their logits and softmax probabilities, and
// the rank of every label.  1 <= k, kmax <= 64, k <= n_cls
// ------------------------------------------------------------------------------------------------
// index [rows, k] = the first k columns of every row in that order; value (may be null) their logits; prob (may be null) the fp32 softmax of
// the WHOLE row at them, summed in a fixed chain: the same bits for a row wherever it lies
int launch_topk(const float* logits, int ldz, int rows, int n_cls, int k, int* index, float* value, float* prob, hipStream_t s);
// state [2 + kmax] int32 = [total, invalid, hist[kmax]]: hist[r] += rows whose label has rank r = the number of columns that precede it; a
// label outside [0, n_cls) only counts as invalid; nothing is reset, launches add up.  rank [rows] (may be null): the full rank, -1 for such a label
int launch_rank_accumulate(const float* logits, int ldz, const int64_t* labels, int rows, int n_cls, int kmax, int* state, int* rank, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// UMuDPT's prompt generator (promptgen.hip; trainers/umudpt.py:56-76,161-178): fp32 end to end, TRAINABLE weights
// ------------------------------------------------------------------------------------------------
// LayerNorm backward that also produces the affine gradients: dx = (dres +) LN'(dy), dgamma[j] (+)= sum_r dy[r][j] xhat[r][j],
// dbeta[j] (+)= sum_r dy[r][j], the row sums in row order (no atomics).  The forward is launch_ln_fwd with out_f32.
struct LnBwdAffineArgs {
    const float* x = nullptr; int ldx = 0;   // LN input rows
    const float* mean = nullptr; const float* rstd = nullptr; const float* gamma = nullptr;  // saved statistics [rows], gamma [d]
    const float* dy = nullptr; int lddy = 0;
    const float* dres = nullptr; int lddres = 0;  // optional residual gradient added to dx
    float* dx = nullptr; int lddx = 0;
    float* dgamma = nullptr; float* dbeta = nullptr; bool accumulate = false;  // accumulate: += instead of = (as launch_colsum)
    int rows = 0, d = 0;
};
int launch_ln_bwd_affine(const LnBwdAffineArgs& a, hipStream_t s);
// fp32 attention on packed qkv [N, L, 3*H*64] (the layout of AttnArgs), 1 <= L <= 16, no mask, q scaled by 1/8; d_model must be H * 64.
// The forward saves the probabilities [N, H, L, L]; the backward reads them and writes dqkv [N, L, 3*H*64].
int launch_pg_attn_fwd(const float* qkv, float* out, float* probs, int N, int L, int H, int d_model, hipStream_t s);
int launch_pg_attn_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int N, int L, int H, int d_model, hipStream_t s);
// y = u sigmoid(1.702 u); du = dy QuickGELU'(u), recomputed from u (du may be dy)
int launch_quickgelu_fwd(const float* u, float* y, size_t n, hipStream_t s);
int launch_quickgelu_bwd(const float* dy, const float* u, float* du, size_t n, hipStream_t s);
// The generator's 18 tensors in ONE flat fp32 buffer, in the reference's named_parameters() order (the bucket's tensors 2 .. 19)
enum PgTensor : int { PG_LN_PRE_G = 0, PG_LN_PRE_B, PG_W_IN, PG_B_IN, PG_W_OUT, PG_B_OUT, PG_LN1_G, PG_LN1_B, PG_W_FC, PG_B_FC, PG_W_PROJ, PG_B_PROJ,
                      PG_LN2_G, PG_LN2_B, PG_LN_POST_G, PG_LN_POST_B, PG_W_VIS, PG_B_VIS, PG_TENSORS };
struct PgParams {
    const float* base = nullptr;
    size_t off[PG_TENSORS] = {}, total = 0;
    const float* at(int i) const { return base + off[i]; }
};
PgParams pg_params(const float* base, int d_t, int d_v);
// activations the backward needs + the backward's scratch, carved from one fp32 buffer of *numel elements (ws null: sizes only)
struct PgWork {
    float *h0 = nullptr, *a1 = nullptr, *qkv = nullptr, *attn = nullptr, *o = nullptr, *y = nullptr, *a2 = nullptr, *u = nullptr, *g = nullptr, *p = nullptr,
          *z = nullptr, *a3 = nullptr, *probs = nullptr, *mean[4] = {}, *rstd[4] = {};
    float *da3 = nullptr, *dz = nullptr, *dg = nullptr, *da2 = nullptr, *dy = nullptr, *dattn = nullptr, *dqkv = nullptr, *da1 = nullptr, *dh0 = nullptr;
};
PgWork pg_carve(float* ws, int depth, int n_ctx, int d_t, size_t* numel);
int pg_check_shape(const char* what, int depth, int n_ctx, int d_t, int d_v);
// G [depth * n_ctx, d_v] from X [depth * n_ctx, d_t]; the backward WRITES the 18 gradients (laid out as the parameters) and dX
int pg_forward(int depth, int n_ctx, int d_t, int d_v, const PgParams& P, const float* X, float* G, const PgWork& w, hipStream_t s);
int pg_backward(int depth, int n_ctx, int d_t, int d_v, const PgParams& P, const float* X, const float* dG, float* dX, float* grads, const PgWork& w, hipStream_t s);

}  // namespace mudpt
