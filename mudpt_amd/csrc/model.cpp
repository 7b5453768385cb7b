// Host side of libmudpt_hip.so: owns the frozen weights and activations in HBM and sequences the
// gfx950 kernels of one MuDPT forward / forward+backward on a HIP stream.
//
// Data layout in HBM (B images, C class prompts, ViT-B/16 numbers in brackets):
//   tokens are batch-first [seq][L][d], never padded: vision L = 1 + P + n_ctx [201], text L = ctx_len [77];
//   the residual stream and its gradient are fp32; GEMM / attention operands (LN output, qkv, attention
//   output, MLP pre-activation, their gradients) are T = bf16 or fp16;
//   frozen Linear weights are stored twice in T: [out,in] for the forward GEMM and [in,out] for the dX GEMM
//   (weights are frozen, so the transposed copy is made once at load; no dW is ever computed);
//   per block the backward needs x_in, x_mid (fp32), LN statistics, qkv, attention output + LSE and the
//   MLP pre-activation: 0.95 GB per block at B = 256, 11.4 GB for the vision tower (288 GB HBM: no recompute).
// Prompt rows are ordinary rows of the token buffer: the reference's torch.cat splices
// (clip/model.py:281-297) are in-place row writes, their backward a fixed-order reduction over the batch.
#include <dlfcn.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/mudpt.h"
#include "kernels.h"

namespace mudpt {

static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* get_error() { return g_err; }

// ---- host-side conversion to the operand dtype -----------------------------------------------------
static inline uint16_t f32_to_bf16(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline uint16_t f32_to_f16(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

// OCP e4m3 (fn: no infinities, maximum 448), round to nearest even, saturating: the weight copies of the e4m3 second pass (common.h LO_F8)
static inline uint8_t f32_to_e4m3(float f) {
    const uint8_t sign = std::signbit(f) ? 0x80 : 0;
    const float a = std::fabs(f);
    if (!(a == a)) return 0x7f;
    if (a >= 464.f) return sign | 0x7e;                   // past the midpoint to the (non-existent) next value: the maximum 448
    if (a <= std::ldexp(1.f, -10)) return sign;           // at most half the smallest subnormal 2^-9: zero (the tie goes to even)
    int e;
    (void)std::frexp(a, &e);                              // a = m 2^e, m in [0.5, 1)
    int E = e - 1 < -6 ? -6 : e - 1;                      // binade (subnormals share 2^-6)
    float r = std::nearbyint(a / std::ldexp(1.f, E - 3)); // in units of 2^(E - 3): [8, 16) normal, [0, 8) subnormal; RNE (default rounding mode)
    if (r >= 16.f) { r = 8.f; E += 1; }
    uint8_t bits = r < 8.f ? (uint8_t)r : (uint8_t)(((E + 7) << 3) | ((int)r - 8));
    if ((bits & 0x7f) == 0x7f) bits = 0x7e;               // 480 would be the NaN code: saturate
    return sign | bits;
}

struct BlockW {
    void *w_in = nullptr, *w_in_t = nullptr, *w_out = nullptr, *w_out_t = nullptr;
    void *w_fc = nullptr, *w_fc_t = nullptr, *w_proj = nullptr, *w_proj_t = nullptr;
    // e4m3 copies of the four forward weights for the second pass of a LO_F8 split tower (common.h): rows of the T copy's length IN BYTES
    // (the first `in` bytes used), values W 2^shift with the per-tensor shift that brings max |W| just below 448; s_* = the MX block scale
    // (E8M0) 2^-shift the matrix instruction applies
    void *w_in8 = nullptr, *w_out8 = nullptr, *w_fc8 = nullptr, *w_proj8 = nullptr;
    int s_in8 = 127, s_out8 = 127, s_fc8 = 127, s_proj8 = 127;
    float *b_in = nullptr, *b_out = nullptr, *b_fc = nullptr, *b_proj = nullptr;
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
};

struct BlockAct {
    float *x_in = nullptr, *x_mid = nullptr;  // fp32 [M, d]
    float *mean1 = nullptr, *rstd1 = nullptr, *mean2 = nullptr, *rstd2 = nullptr;
    void *qkv = nullptr, *attn = nullptr, *u = nullptr;  // T
    float* lse = nullptr;
};

// The text tower's sequence layout for one set of class prompts (plan_text_layout is the rule, fill_layout_tables makes the device tables,
// bind_text_layout points the tower at one).  Length buckets (many classes): the sequences are sorted by length and packed bucket after bucket,
// each bucket with its own row count per sequence, so the row-wise kernels (GEMMs, LayerNorm) run once over `rows` packed rows while the
// kernels that know about sequences (attention, prompt splice, prompt-row reductions) run once per bucket.
struct TextLayout {
    struct Seg { int row0 = 0, seq0 = 0, nseq = 0, L = 0; size_t lse0 = 0; };  // first packed row / sequence, sequences, rows per sequence, offset into the LSE buffers
    std::vector<Seg> segs;          // the buckets, at least one; one bucket keeps the caller's order
    int rows = 0, L = 0, nseq = 0;  // packed rows, longest kept length, sequences per pass (CoCoOp: a chunk of images x n_cls)
    int *eot_rows = nullptr, *eot_local = nullptr, *perm = nullptr;  // device: EOT row of every sequence, packed / relative to its bucket; packed position -> class
    bool packed() const { return segs.size() > 1; }
};

struct Tower {
    int d = 0, layers = 0, heads = 0, L = 0, max_seq = 0, Lp = 0;  // L, Lp: rows per sequence (text: the bound layout's longest kept length), padded for attention
    bool causal = false;
    // Split operands (common.h LoMode).  The forward GEMMs' A operands -- both LayerNorm outputs, the attention output and QuickGELU(u) --
    // are stored as hi = T(v) plus the remainder lo in a second buffer, and the GEMM contracts lo in a second pass: against the same
    // weights (LO_F16: 22 bits; CLIP's weights are fp16-exact, checkpoints are fp16-stored) or, as e4m3 bytes, against an e4m3 copy of
    // the weights on the fp8 matrix pipe (LO_F8: ~15 bits at half the cost of the pass).  Which the modes use, and what each site buys:
    // DESIGN.md 2 (tests/precision_ablation.py: the text tower needs every bit at every site, the vision tower's error is c_fc / c_proj first).
    int split = LO_NONE;
    bool may_split = false;   // low-half buffers (and, vision tower, the e4m3 weights) exist: split / sites / exact_attn are knobs
    int sites = 0x1f;         // knob: sites that take part -- bit 0 ln_1 -> in_proj, 1 attention -> out_proj, 2 ln_2 -> c_fc, 3 QuickGELU -> c_proj, 4 pixels -> patch embed
    void *h_lo = nullptr, *g_lo = nullptr, *attn_lo = nullptr;               // low halves of h, g, the attention output: rows of 2 d / 8 d / 2 d bytes
    void *h_sel_lo = nullptr, *g_sel_lo = nullptr, *attn_sel_lo = nullptr;   // ... of the last block's tail
    int prompt_row0 = 0;  // first prompt row inside a sequence (vision: L - n, text: 1)
    // Prompt rows per sequence and deep-prompt layers of THIS tower: blocks 1 .. D1 splice n rows.  MuDPT / CoCoOp / CoOp: both towers
    // from mudpt_config (n_ctx, depth - 1; the vanilla vision tower of CoCoOp / CoOp has none); VPT / MPT: mudpt_prompt_shape, per tower
    int n = 0, D1 = 0;
    std::vector<BlockW> w;
    std::vector<BlockAct> a;  // layers entries; the last block's output exists on the tail rows only (xout_sel)
    // scratch shared by all blocks
    void *h = nullptr, *g = nullptr;                    // T [M,d], T [M,4d]
    // Attention forward in fp32 (attention_exact.hip; the parity mode's text tower, knob for its vision tower): in_proj writes q | k | v in
    // fp32 to qkv32, the attention kernel leaves the fp16 copy the backward reads.
    bool exact_attn = false;
    float* qkv32 = nullptr;                             // fp32 [M, 3d] scratch (allocated when may_split && the mode is MUDPT_F32)
    float* dx = nullptr; void* dx_lp = nullptr;         // gradient residual stream fp32 + T copy
    void *dattn = nullptr, *dqkv = nullptr;             // T
    float* delta = nullptr;
    float* upd = nullptr;  // fp32 [M, d]: out_proj / c_proj result, added to the stream by the next LayerNorm kernel
    // Tail of the last block.  Only ONE row per sequence of the last block's output is ever used (the CLS token,
    // clip/model.py:549, or the EOT token, trainers/mudpt.py:154), so everything after that block's attention -- out_proj,
    // ln_2, the MLP, the residual adds and their backward -- runs on those max_seq rows only ("sel": compact [max_seq, *]).
    // Results are identical to the reference's: the other rows of its last block output are computed and dropped.
    const int* tail_rows = nullptr;  // [nseq] token row (b * L + position) of the used row of every sequence
    float *xin_sel = nullptr, *xmid_sel = nullptr, *xout_sel = nullptr;  // fp32 [S, d]
    void *attn_sel = nullptr, *h_sel = nullptr, *u_sel = nullptr, *g_sel = nullptr, *dattn_sel = nullptr;  // T
    float* dsel = nullptr; void* dsel_lp = nullptr;  // gradient of the residual stream on the selected rows (fp32 / T)
    // single-query attention of the last block (attention_single.hip): the one query per sequence, its gradient, its log-sum-exp
    void *q_sel = nullptr, *dq_sel = nullptr, *dqx_sel = nullptr;  // T [S, d]
    float* lse_sel = nullptr;                                       // [S, heads]
    // Head of the backward pass: block 0's input gradient is only needed on the n_ctx prompt rows of every sequence (the
    // other rows of the tower input have no trainable ancestor), so its in_proj dX GEMM and ln_1 backward run on those rows.
    const int* head_rows = nullptr;  // [nseq * n_ctx] token rows of the prompt tokens
    int head_n = 0;                  // rows per sequence
    int head_span = 0;               // rows prompt_row0 .. prompt_row0 + head_span - 1 hold every head row (0 = head_n; CoOp middle / front: wider)
    void *hd_dqkv = nullptr, *hd_h = nullptr;  // T [max_seq * n_ctx, 3 d], [max_seq * n_ctx, d]
    std::vector<void*> act_allocs;  // activation / scratch buffers (sized for max_seq sequences of L rows): re-made when L changes
    typedef TextLayout::Seg Seg;
    const TextLayout* lay = nullptr;  // text tower: the bound layout (bind_text_layout); the vision tower has none
    bool packed() const { return lay && lay->packed(); }
};

// rows of a tower pass over nseq sequences; its buckets: the bound layout's as they lie when it is packed, else one pseudo-bucket of
// nseq x L (the vision tower's batch, CoCoOp's chunk)
static int tower_rows(const Tower& t, int nseq) { return t.packed() ? t.lay->rows : nseq * t.L; }
struct TowerSegs {
    Tower::Seg one;
    const Tower::Seg *b = &one, *e = &one + 1;
    TowerSegs(const Tower& t, int nseq) { one.nseq = nseq; one.L = t.L; if (t.packed()) { b = t.lay->segs.data(); e = b + t.lay->segs.size(); } }
    TowerSegs(const TowerSegs&) = delete;
    const Tower::Seg* begin() const { return b; } const Tower::Seg* end() const { return e; }
};

// One trainable tensor: the reference's state-dict key, its shape (ndim extents, the rest 0) and its place in the flat bucket (elements)
struct Trainable {
    std::string name;
    int ndim = 0;
    int64_t shape[3] = {0, 0, 0};
    size_t off = 0, numel = 0;
};

// ---- CLIP's ResNet image tower (mudpt_create_frozen_resnet, mudpt_create_resnet; clip/model.py:17-161; kernels: resnet.hip) ----
// One bias-free convolution and the eval-mode BatchNorm behind it, folded into one GEMM B operand + fp32 bias (mudpt_conv_pack)
struct RnConv {
    std::string conv, bn;  // state-dict prefixes: conv + ".weight"; bn + ".weight" / ".bias" / ".running_mean" / ".running_var"
    int cin = 0, cout = 0, k = 1;
    int ldk = 0;  // the GEMM's K: k k cin rounded up to 64, zero-filled in the packed weights (and in the patch rows / the padded channels of A)
    int np = 0;   // the GEMM's N and the output's channel stride: cout, rounded up to 64 where a 1 x 1 convolution reads the output as its A
                  // operand as it lies (width 32: K = 32) -- the extra weight rows and biases are zero, so the extra channels are written as zeros
    std::vector<float> w, bnp[4];  // fp32 host copies as uploaded: w [cout, cin, k, k]; gamma, beta, running_mean, running_var [cout]
    void* w_dev = nullptr;         // T [np, ldk], column (ky * k + kx) * cin + c
    float* b_dev = nullptr;        // [np]
};
struct RnBlock { int conv1 = 0, conv2 = 0, conv3 = 0, down = -1, stride = 1; };  // indices into Resnet::convs; down = -1: the identity is the input
struct Resnet {
    mudpt_resnet_shape shape;
    int S = 0, C = 0, L = 0;  // image size; output channels 32 width; tokens of the attention pool (S / 32)^2 + 1
    std::vector<RnConv> convs;  // 0, 1, 2: the stem
    std::vector<RnBlock> blocks;
    bool stale = true;  // a "visual.*" tensor arrived since the last fold
    int conv_path = 0;  // mudpt_resnet_conv_path: 0 = im2col + GEMM + bias_act per convolution, 1 = one launch_conv2d (conv.hip)
    long conv2d_launches = 0;  // launch_conv2d calls of the tower since create (mudpt_debug_read "conv2d_launches"): path 0 adds none
    float *pos = nullptr, *b_q = nullptr, *b_kv = nullptr, *b_c = nullptr;  // attnpool: positional_embedding [L, C]; biases [C], [2 C] (k | v), [e]
    void *w_q = nullptr, *w_kv = nullptr, *w_c = nullptr;                   // T [C, C], [2 C, C] (k_proj over v_proj), [e, C]
    // activations, sized for max_batch at create (bytes for RN50 at B 100: DESIGN.md 4.9)
    void* act[7] = {};     // T NHWC: block input, block output, conv1 / conv2 outputs, pooled conv2 output, downsample branch, pooled block input
    void* rows = nullptr;  // T patch rows of the largest 3 x 3 convolution
    float* acc = nullptr;  // fp32 output of the largest convolution GEMM
    void *tok = nullptr, *ao = nullptr;  // T [B, L, C] pooled tokens, [B, C] attention output
    float *q = nullptr, *kv = nullptr;   // fp32 [B, C], [B L, 2 C]
};

}  // namespace mudpt

using namespace mudpt;

struct mudpt_model {
    mudpt_config cfg;
    int dtype = 0;
    bool exact = false;  // mudpt_config.dtype == MUDPT_F32: fp16 split operands everywhere on the forward + fp32 attention forward
    std::vector<void*> allocs;
    std::vector<std::string> missing;  // weight keys not yet set
    bool prompts_set = false;
    bool text_valid = false;  // txt_f holds the text features of the currently bound parameter values' last forward
    int feat_B = 0;           // img_f holds the raw features of the last INFERENCE forward, of this many images (mudpt_image_features); 0: of none

    Tower vis, txt;
    // vision stem / head
    void* conv_w = nullptr;  // T [dv, K0]
    void* conv_w8 = nullptr; int conv_s8 = 127;  // parity mode: its e4m3 copy (rows of 2 K0 bytes) + block scale, BlockW::w_in8
    void* patches_lo = nullptr;                  // ... and the low halves of the pixels
    float *cls = nullptr, *vpos = nullptr, *ln_pre_g = nullptr, *ln_pre_b = nullptr, *ln_post_g = nullptr, *ln_post_b = nullptr;
    float* vproj = nullptr;  // [dv, e]
    void* patches = nullptr; // T [B P, 3 p p]
    float *xpre = nullptr, *pre_mean = nullptr, *pre_rstd = nullptr;
    float *f_ln = nullptr, *post_mean = nullptr, *post_rstd = nullptr, *df_ln = nullptr;
    int *cls_rows = nullptr, *vprompt_rows = nullptr;
    // text stem / head
    float *tpos = nullptr, *ln_fin_g = nullptr, *ln_fin_b = nullptr, *tproj = nullptr;
    float* emb_pos = nullptr;  // [C, Lt, dt] class token embeddings + positional embedding
    int* tprompt_rows = nullptr;
    TextLayout lay;  // of the class prompts (mudpt_set_class_prompts); its device tables are allocated at create.  Frozen handles: Template::lay
    float *txt_sorted = nullptr, *dtxt_sorted = nullptr;  // [C, e] text features / their gradient in packed (length-sorted) order
    float *t_ln = nullptr, *fin_mean = nullptr, *fin_rstd = nullptr, *dt_ln = nullptr;
    float scale = 1.f;
    // prompt learner intermediates (fp32)
    float *shared = nullptr, *t2v = nullptr, *v2t = nullptr, *vis_deep = nullptr, *txt_deep = nullptr;
    float *d_vis_deep = nullptr, *d_txt_deep = nullptr, *d_vprompt0 = nullptr;
    float* vsplice = nullptr;  // [max_batch][(depth - 1) n_ctx][dv] fp32: per-image gradients of the spliced vision prompt rows (vision_backward)
    // head
    float *img_f = nullptr, *txt_f = nullptr, *img_n = nullptr, *txt_n = nullptr, *img_inv = nullptr, *txt_inv = nullptr;
    float *logits = nullptr, *dlogits = nullptr, *row_loss = nullptr, *dimg = nullptr, *dtxt = nullptr, *loss = nullptr;
    // parameters
    float *params = nullptr, *grads = nullptr, *momentum = nullptr;
    bool sgd_first = true;
    // The variant's trainables in the reference's named_parameters() order (build_trainables): the layout of the flat bucket and what
    // mudpt_param_info reports.  The one source of names, shapes and offsets (elements)
    std::vector<Trainable> tr;
    size_t off(int i) const { return tr[i].off; }
    size_t total = 0;
    // CoCoOp variant (trainers/cocoop.py): 5 trainables, vanilla vision tower (forward only), B * C text sequences
    bool cocoop = false;
    // Class-parallel text tower (second axis): this handle encodes classes [c0, c0 + ct) of the n_cls only; the
    // [n_cls, e] text-feature table is completed by the caller's exchange between the mudpt_cp_* phases.  Default: all classes.
    int c0 = 0, ct = 0;
    bool sharded = false;
    float cp_unscale = 0.f;  // of the step in flight between mudpt_cp_head and mudpt_cp_backward
    int cp_B = 0, cp_stage = 0;  // 1 = towers forward done, 2 = head (training) done
    int cl_B = 0;  // images of the mudpt_forward_train whose activations and head state are still in place (mudpt_backward_logits); 0: of none
    int64_t cl_serial = 0;  // number of that forward (mudpt_train_token): 1, 2, ... over the handle's life
    int hid = 0;  // meta_net hidden width = embed_dim / 16 (trainers/cocoop.py:104)
    // CoOp variant (trainers/coop.py): 1 trainable (ctx, shared or one per class with CSC), vanilla vision tower (forward only), C text
    // sequences as MuDPT.  The context rows of class c sit at prompt positions coop_pos[c * n ..] (CLASS_TOKEN_POSITION); tprompt_rows
    // then holds their token rows in the CALLER's class order (coop.hip)
    bool coop = false, csc = false;
    int class_token_position = MUDPT_CLASS_TOKEN_END;
    std::vector<int> name_lens;  // [n_cls] (trainers/coop.py:80); empty = all 0 (END without lengths)
    int* coop_pos = nullptr;     // [n_cls * n_ctx] device
    // VPT / MPT variants (trainers/vpt.py, mpt.py): every spliced prompt is a trainable of its own, so block i's rows come straight from
    // the bound bucket and their gradients go straight into the gradient bucket (prompt_route); no prompt-learner GEMMs
    bool vpt = false, mpt = false, indep = false;  // indep = vpt || mpt: independent prompts per tower
    int tr_txt0 = 0, tr_vis0 = 0;  // ... and the table index of each tower's first tensor (build_trainables)
    // UMuDPT variant (trainers/umudpt.py): MuDPT's towers; the bucket holds ctx, deep_prompts and the 18 tensors of the prompt generator
    // (promptgen.hip).  X = cat(ctx, deep_prompts) is the bucket's first depth * n_ctx rows as they lie; G = generator(X) [depth, n, dv] feeds the
    // vision tower (row group 0: the input prompt rows, 1..: the deep prompts), pg_dG collects its gradient from the vision tower's backward
    bool umudpt = false;
    float *pg_G = nullptr, *pg_dG = nullptr, *pg_dX = nullptr, *pg_ws = nullptr;
    PgWork pg_w;
    // UUMuDPT variant (trainers/uumudpt.py): UMuDPT (umudpt is set too: Gen1 and everything above serve both) plus the other direction.  The
    // vision tower owns visual_ctx, visual_ctx_deep_prompts and a SECOND generator of width dv (clip/model.py:600-664) behind Gen1's tensors in
    // the bucket: vision input rows G[0] + visual_ctx, vision deep prompts vis_deep = G[1:] + visual_ctx_deep_prompts, text deep prompts
    // txt_deep = deep_prompts + T with T = Gen2(visual_ctx_deep_prompts) [depth - 1, n, e]; d_txt_deep is dT.  Gen2 idles at depth 1
    bool uumudpt = false;
    float *pg2_T = nullptr, *pg2_ws = nullptr;
    PgWork pg2_w;
    // Frozen CLIP (mudpt_create_frozen; trainers/zsclip.py): no trainable, both towers vanilla and forward only.  The class prompts arrive as token
    // ids (mudpt_set_text_tokens), one set per prompt template; every template has its own packed text layout and two device tables (token id,
    // position) per token row, and the text tower runs once per template from the device-resident embedding table.  txt_n holds the ensembled,
    // normalised features (text_valid), the only thing a forward needs from the text side
    bool frozen = false;
    Resnet* rn = nullptr;  // mudpt_create_frozen_resnet, mudpt_create_resnet: the image tower is this instead of `vis`, which then has no block
    float* tok_table = nullptr; int vocab = 0;// "token_embedding.weight" fp32 [vocab, t_width]
    struct Template {
        TextLayout lay;                            // its device tables inside tmpl_tables
        const int *tok = nullptr, *pos = nullptr;  // device, inside tmpl_tables: token id and position of every packed token row
    };
    std::vector<Template> tmpl;
    int* tmpl_tables = nullptr;  // one allocation behind every Template's tables
    float* ens_acc = nullptr;    // [n_cls, e] running sum of the normalised per-template features
    long text_launches = 0;  // text-tower passes + text-side head launches (mudpt_debug_read "text_launches")
    float *mn_hid = nullptr, *mn_bias = nullptr, *mn_dbias = nullptr, *mn_dhid = nullptr;  // [B, hid], [B, dt], [B, dt], [B, hid]
    float loss_scale = 128.f;  // static, power of two; see mudpt_forward_backward
    // bf16 mode keeps the gradient of the residual stream in T only (the fp32 copy costs 237 MB of HBM traffic per LayerNorm
    // backward); fp16 mode -- the parity configuration -- keeps it in fp32.  mudpt_model_set("lp_grad", 1) moves fp16 mode to fp16
    // activation gradients as well (what the reference's own fp16 model has; the static loss scale keeps them normal): measured on
    // the fixtures, logits unchanged (forward only), gradient errors +30 % (ViT-B/16 worst max-error 1.8e-2 -> 2.5e-2 of the tensor's
    // RMS; CoCoOp's meta_net gradients reach the edge of the test's error model), step 26.5 -> 25.6 ms.  Not the default: the parity
    // mode exists for accuracy.
    bool lp_grad = false;
    // bf16 mode: c_fc stores QuickGELU'(u) in 8 bits for the backward instead of u in T (common.h gelu_grad_q8x4): -158 MB written and
    // -158 MB read per MLP and step at an error of 2.4e-3 on a factor in [-0.1, 1.1] -- bf16's own grade.  Knob gelu_q8.
    bool gelu_q8 = false;
    bool lp_upd = false;   // the forward's update stream (out_proj / c_proj results added by the next LayerNorm) in T instead of fp32: bf16 mode
    // per-handle tuning knobs (mudpt_model_set): nothing here is process-global, two models in one process do not interfere
    int gemm_variant = 0;
    bool txt_trim = true;  // run the text tower on positions 0..max(eot) only (read by mudpt_set_class_prompts)
    int txt_bucket_cost = 1024;  // knob: what one more bucket costs in the cut search, in token rows (its extra launches per block)
    int txt_buckets = 3;   // knob: at most this many length buckets for the class prompts (1 = every prompt runs to the longest EOT)
    bool attn_fused_w1 = false;
    bool split_k = true;      // knob: split K for the small-grid, long-K store GEMMs (small batches)
    bool fwd_split_k = true;  // knob: ... of the forward too, up to kFwdSplitTiles tiles (gemm_call) -- in a TRAINING step's forward only
    bool train_fwd = false;   // the forward in flight belongs to a training step (mudpt_forward_backward, mudpt_cp_forward with MUDPT_FWD_TRAINING):
                              // inference forwards never split K, so eval logits of an image do not depend on the size of its (last, partial) test batch
    static constexpr size_t kFwdSplitTiles = 320;
    static constexpr size_t kScratchElems = (size_t)4 << 20;  // 4 slices x 128 tiles of 128 x 64 fp32
    float *gemm_scratch = nullptr, *gemm_scratch2 = nullptr;
    bool attn_window = true;  // knob: block 0's attention backward computes the 16-row blocks of the prompt rows only (0 = all rows)
    bool last_single = true;  // knob: single-query attention in the last block (0 = the general kernels on all rows)
    bool attn_two_kernels = false;  // knob: attention backward as the dQ + dK/dV kernel pair instead of the fused single pass
    int cocoop_chunk = 0;  // knob: cap on the images per text-tower pass (0 = as many as the memory budget allows)
    int txt_chunk = 1;     // CoCoOp: images per text-tower pass, set by mudpt_set_class_prompts
    bool any_weight_set = false;
    // side stream for the text tower (forks after the prompt learner / head backward, joins before the head /
    // prompt-learner backward)
    hipStream_t s2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fork_b = nullptr, ev_join_b = nullptr;
    // optional HIP-event timing of the big vision-tower launches (bench.py's roofline legs), by kernel class
    bool prof = false;
    int prof_mask = 0;  // bit c: launches of class c are bracketed (an event pair costs ~5 us of queue time per launch)
    int prof_stride = 1;  // knob: every prof_stride-th gemm_pp launch is bracketed (launch counter runs across steps: with a launch
                          // count per step coprime to the stride, every launch site is sampled equally often over `stride` steps)
    long pp_seen = 0;
    std::vector<hipEvent_t> ev;  // pairs
    size_t ev_used = 0;
    struct ProfRec { int cls; double work; };
    std::vector<ProfRec> ev_rec;  // one per event pair: class and algorithmic work (FLOPs for the GEMM, bytes for the HBM-bound kernels)
    double exec_flop = 0;         // executed MFMA FLOPs (every GEMM and attention launch of both towers) since profile_enable / read
};
enum ProfClass : int { PC_GEMM = 0, PC_LN_FWD = 1, PC_LN_BWD = 2, PC_ATTN_FWD = 3, PC_ATTN_BWD = 4, PC_COUNT = 5 };

// Next event pair for a bracketed launch of class cls (nullptr-filled when profiling is off).
static int prof_next(mudpt_model* m, int cls, double work, LaunchProf* out) {
    *out = LaunchProf();
    if (!m->prof || !(m->prof_mask & (1 << cls))) return MUDPT_OK;
    if (m->ev_used + 2 > m->ev.size()) {
        for (int i = 0; i < 512; ++i) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            m->ev.push_back(e);
        }
    }
    out->start = m->ev[m->ev_used];
    out->stop = m->ev[m->ev_used + 1];
    m->ev_used += 2;
    m->ev_rec.push_back({cls, work});
    return MUDPT_OK;
}

// Every MFMA GEMM of the path goes through here; with profiling on, the launch is bracketed by HIP events on
// the launch stream and its algorithmic FLOPs (2 M N K) are recorded.
// bwd: a GEMM of the backward pass.  Those may always split K; a FORWARD GEMM only where the caller allows it (fwd_split: the vision
// tower's out_proj / c_proj, never with split operands) and its grid is at most kFwdSplitTiles 64 x 64 tiles (ViT-B: up to 8 images -- the
// reference's own training batch of 4, where c_proj's 48-step chain on 156 workgroups was the longest kernel of the step).  The text
// tower never splits, forward or backward (its call sites pass bwd = !t.causal): its features are bit-identical and its gradients equal to
// the order of the fp32 sums over classes however the class prompts are bucketed (a tested property; a split decision that depends on the
// row count of a bucketing moved the fp16 gradients by 1e-2 of their rms, the size of the fp16 backward's whole rounding noise).  A split sum has a different fp32 association than the sequential one and whether a shape splits depends on M, so the
// tested property "logits of a batch equal the logits of its chunks bit for bit" holds for chunks ABOVE that size (knob fwd_split_k = 0
// restores it for every size); gradients are only held to agree to rounding.
static int gemm_call(mudpt_model* m, int epi, const GemmArgs& a, hipStream_t s, bool bwd = false, bool fwd_split = false) {
    // only the dominant kernel is bracketed: gemm_pp_kernel launches (the vision tower's big GEMMs, main stream).  The text
    // tower's small GEMMs run on the side stream, where an event pair would mostly measure queueing behind the other stream.
    GemmOpts o;
    o.variant = m->gemm_variant;
    const bool fwd_small = fwd_split && m->fwd_split_k && m->train_fwd && (size_t)((a.M + 63) / 64) * ((a.N + 63) / 64) <= mudpt_model::kFwdSplitTiles;
    if (m->split_k && (bwd || fwd_small)) {  // split-K partials: one scratch per stream (the towers run concurrently)
        o.scratch = s == m->s2 ? m->gemm_scratch2 : m->gemm_scratch;
        o.scratch_elems = mudpt_model::kScratchElems;
    }
    if (m->prof) m->exec_flop += 2.0 * a.M * a.N * a.K;
    if (!m->prof || !gemm_uses_pp(epi, a, o.variant)) return launch_gemm(m->dtype, epi, a, s, o);
    if (m->prof_stride > 1 && (m->pp_seen++ % m->prof_stride) != 0) return launch_gemm(m->dtype, epi, a, s, o);
    LaunchProf lp;
    if (int rc = prof_next(m, PC_GEMM, 2.0 * a.M * a.N * a.K, &lp)) return rc;
    o.ev_start = lp.start;
    o.ev_stop = lp.stop;
    return launch_gemm(m->dtype, epi, a, s, o);
}

// LayerNorm / attention launches of the path.  The big vision-tower ones (main stream) are bracketed when profiling is on; their
// work figure is the ALGORITHMIC HBM bytes of the launch: every operand read once, every result written once.
static bool prof_big(const mudpt_model* m, const Tower& t, int rows) { return m->prof && &t == &m->vis && rows >= 4096; }
static int ln_fwd_call(mudpt_model* m, const Tower& t, const LnFwdArgs& a, hipStream_t s) {
    if (!prof_big(m, t, a.rows)) return launch_ln_fwd(m->dtype, a, s);
    const double per_elem = 4.0 + (a.add ? 4.0 : 0.0) + (a.add_lp ? 2.0 : 0.0) + (a.xout ? 4.0 : 0.0) + (a.out_f32 ? 4.0 : 2.0) + (a.out_lo ? 2.0 : 0.0);
    LaunchProf lp;
    if (int rc = prof_next(m, PC_LN_FWD, per_elem * a.rows * a.d, &lp)) return rc;
    return launch_ln_fwd(m->dtype, a, s, &lp);
}
static int ln_bwd_call(mudpt_model* m, const Tower& t, const LnBwdArgs& a, hipStream_t s) {
    if (!prof_big(m, t, a.rows)) return launch_ln_bwd(m->dtype, a, s);
    const double per_elem = (a.dy_f32 ? 4.0 : 2.0) + 4.0 + (a.dres ? 4.0 : 0.0) + (a.dres_lp ? 2.0 : 0.0) + (a.dx ? 4.0 : 0.0) + (a.dx_lp ? 2.0 : 0.0);
    LaunchProf lp;
    if (int rc = prof_next(m, PC_LN_BWD, per_elem * a.rows * a.d, &lp)) return rc;
    return launch_ln_bwd(m->dtype, a, s, &lp);
}
static int attn_call(mudpt_model* m, const Tower& t, const AttnArgs& a, bool bwd, hipStream_t s) {
    AttnOpts o;
    o.two_kernels = m->attn_two_kernels;
    o.fused_w1 = m->attn_fused_w1;
    // executed MFMA FLOPs: forward S = QK^T and PV (2 products of 2 L^2 64 each per head); backward 7 products (dQ sweep: S, dP, dQ;
    // dK/dV sweep: S, dP, dV, dK); the causal tower does about half of each
    const double prod = 2.0 * a.L * (double)a.L * 64.0 * a.H * a.B * (a.causal ? 0.5 : 1.0);
    const bool exact_fwd = !bwd && a.qkv32;  // fp32 attention forward: fp32 matrix-core FLOPs are not counted as executed bf16 / fp16 MFMA work
    if (m->prof && !a.sel_rows && !exact_fwd) m->exec_flop += (bwd ? 7.0 : 2.0) * prod;
    if (exact_fwd) return launch_attn_fwd_exact(a, s);
    if (!prof_big(m, t, a.B * a.L) || a.sel_rows) return bwd ? launch_attn_bwd(m->dtype, a, s, o) : launch_attn_fwd(m->dtype, a, s, o);
    // algorithmic bytes: forward reads q, k, v and writes o (+ its low half in split mode); backward reads q, k, v, o, do and writes dq, dk, dv
    const double tok = (double)a.B * a.L * a.H * 128.0;
    LaunchProf lp;
    if (int rc = prof_next(m, bwd ? PC_ATTN_BWD : PC_ATTN_FWD, bwd ? 8.0 * tok : (4.0 + (a.out_lo ? 1.0 : 0.0)) * tok, &lp)) return rc;
    o.prof = &lp;
    return bwd ? launch_attn_bwd(m->dtype, a, s, o) : launch_attn_fwd(m->dtype, a, s, o);
}

// Indices into mudpt_model::tr, the table of the variant they belong to (build_trainables): P_* MuDPT (UMuDPT shares P_CTX, P_DEEP),
// Q_* CoCoOp, U_GEN the first of the UMuDPT generator's 18 tensors (kernels.h PgTensor), UU_* what UUMuDPT adds behind those
enum { P_CTX = 0, P_DEEP, P_EW, P_EB, P_DW, P_DB, P_VCTX, P_VDEEP, P_VW, P_VB };
enum { Q_CTX = 0, Q_W1, Q_B1, Q_W2, Q_B2 };
enum { U_GEN = 2 };
enum { UU_VCTX = 20, UU_VDEEP, UU_GEN2 };  // UUMuDPT behind UMuDPT's 20: visual_ctx, visual_ctx_deep_prompts, the first of Gen2's 18 tensors

// The variant's trainables: the reference's key and shape of every tensor, in its named_parameters() order -- the flat bucket's layout
static void build_trainables(mudpt_model* m) {
    const mudpt_config& c = m->cfg;
    const int64_t n = c.n_ctx, D1 = c.depth - 1, dt = c.t_width, dv = c.v_width, e = c.embed_dim, hd = e / 16;
    auto add = [&](const std::string& name, std::initializer_list<int64_t> shape) {
        Trainable t;
        t.name = name; t.ndim = (int)shape.size(); t.off = m->total; t.numel = 1;
        std::copy(shape.begin(), shape.end(), t.shape);
        for (int64_t x : shape) t.numel *= (size_t)x;
        m->total += t.numel;
        m->tr.push_back(t);
    };
    if (m->cocoop) {  // names under CustomCLIP (trainers/cocoop.py:96-107,176; the reference registers the prompt_learner sub-module)
        add("prompt_learner.ctx", {n, dt});
        add("prompt_learner.meta_net.linear1.weight", {hd, e});
        add("prompt_learner.meta_net.linear1.bias", {hd});
        add("prompt_learner.meta_net.linear2.weight", {dt, hd});
        add("prompt_learner.meta_net.linear2.bias", {dt});
    } else if (m->coop) {  // the one trainable under CustomCLIP (trainers/coop.py:60-76,206; only prompt_learner is registered, :255-259)
        if (m->csc) add("prompt_learner.ctx", {c.n_cls, n, dt});
        else add("prompt_learner.ctx", {n, dt});
    } else if (m->indep) {
        // VPT / MPT: every visual_ctx [n, width] in the reference's named_parameters() order (text_prompt_learner, text_encoder, image_encoder;
        // clip/model.py:202-251); a tower's tensors follow one another, so its blocks' are the [D1][n][width] array the splice and the
        // gradient reductions address
        if (m->mpt) {
            m->tr_txt0 = (int)m->tr.size();
            add("text_prompt_learner.visual_ctx", {m->txt.n, dt});  // trainers/mpt.py:86
            for (int i = 1; i <= m->txt.D1; ++i) add("text_encoder.transformer.resblocks." + std::to_string(i) + ".visual_ctx", {m->txt.n, dt});
        }
        if (m->vis.n > 0) {
            m->tr_vis0 = (int)m->tr.size();
            add("image_encoder.visual_ctx", {m->vis.n, dv});  // clip/model.py:459-465
            for (int i = 1; i <= m->vis.D1; ++i) add("image_encoder.transformer.resblocks." + std::to_string(i) + ".visual_ctx", {m->vis.n, dv});
        }
    } else if (m->umudpt) {
        // trainers/umudpt.py:110-124: ctx, deep_prompts ([0, n, dt] at depth 1: no elements, still listed), then the generator.  UUMuDPT
        // (trainers/uumudpt.py:111-125, clip/model.py:606-628): the same 20 under its own prefix, then the vision tower's 20.
        // generator: the 18 tensors of one generator of width d (kernels.h PgTensor) -- ln_pre, the block, ln_post, the output Linear
        auto generator = [&](const std::string& p, const std::string& a, const std::string& post, const std::string& proj, int64_t d, int64_t d_out) {
            add(p + ".weight", {d});
            add(p + ".bias", {d});
            add(a + "attn.in_proj_weight", {3 * d, d});
            add(a + "attn.in_proj_bias", {3 * d});
            add(a + "attn.out_proj.weight", {d, d});
            add(a + "attn.out_proj.bias", {d});
            add(a + "ln_1.weight", {d});
            add(a + "ln_1.bias", {d});
            add(a + "mlp.c_fc.weight", {4 * d, d});
            add(a + "mlp.c_fc.bias", {4 * d});
            add(a + "mlp.c_proj.weight", {d, 4 * d});
            add(a + "mlp.c_proj.bias", {d});
            add(a + "ln_2.weight", {d});
            add(a + "ln_2.bias", {d});
            add(post + ".weight", {d});
            add(post + ".bias", {d});
            add(proj + ".weight", {d_out, d});
            add(proj + ".bias", {d_out});
        };
        const std::string p = m->uumudpt ? "uumudpt_prompt_learner." : "umudpt_prompt_learner.";
        add(p + "ctx", {n, dt});
        add(p + "deep_prompts", {D1, n, dt});
        generator(p + "ln_pre", p + "self_attn.", p + "ln_post", p + "visual_proj", dt, dv);
        if (m->uumudpt) {
            const std::string v = "image_encoder.visual_ctx";
            add(v, {n, dv});
            add(v + "_deep_prompts", {D1, n, dv});
            generator(v + "_ln_intra_pre", v + "_self_attn.", v + "_ln_intra_post", v + "_text_proj", dv, e);
        }
    } else {  // MuDPT: trainers/mudpt.py:71-81, clip/model.py:512-519
        add("mudpt_prompt_learner.ctx", {n, dt});
        add("mudpt_prompt_learner.deep_prompts", {D1, n, dt});
        add("mudpt_prompt_learner.embed_projection.weight", {dv, dt});
        add("mudpt_prompt_learner.embed_projection.bias", {dv});
        add("mudpt_prompt_learner.deep_projections.weight", {dv, dt});
        add("mudpt_prompt_learner.deep_projections.bias", {dv});
        add("image_encoder.visual_ctx", {n, dv});
        add("image_encoder.visual_ctx_deep_prompts", {D1, n, dv});
        add("image_encoder.visual_ctx_deep_projections.weight", {e, dv});
        add("image_encoder.visual_ctx_deep_projections.bias", {e});
    }
}


static int dev_alloc(mudpt_model* m, void** out, size_t bytes) {
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, bytes ? bytes : 16));
    m->allocs.push_back(p);
    *out = p;
    return MUDPT_OK;
}
#define ALLOC(ptr, bytes)                                              \
    do {                                                               \
        if (int _e = dev_alloc(m, (void**)&(ptr), (size_t)(bytes))) return _e; \
    } while (0)

// Frozen weights of a tower (device copies; filled by mudpt_set_weight).
static int alloc_tower_weights(mudpt_model* m, Tower& t, int d, int layers, int heads, bool causal, int prompt_row0, bool f8_weights) {
    t.d = d; t.layers = layers; t.heads = heads; t.causal = causal; t.prompt_row0 = prompt_row0;
    t.w.resize(layers);
    t.a.resize(layers);
    for (int i = 0; i < layers; ++i) {
        BlockW& w = t.w[i];
        ALLOC(w.w_in, (size_t)3 * d * d * 2); ALLOC(w.w_in_t, (size_t)3 * d * d * 2);
        ALLOC(w.w_out, (size_t)d * d * 2); ALLOC(w.w_out_t, (size_t)d * d * 2);
        ALLOC(w.w_fc, (size_t)4 * d * d * 2); ALLOC(w.w_fc_t, (size_t)4 * d * d * 2);
        ALLOC(w.w_proj, (size_t)4 * d * d * 2); ALLOC(w.w_proj_t, (size_t)4 * d * d * 2);
        if (f8_weights) {  // e4m3 copies at the T copies' row length in bytes
            ALLOC(w.w_in8, (size_t)3 * d * d * 2); ALLOC(w.w_out8, (size_t)d * d * 2);
            ALLOC(w.w_fc8, (size_t)4 * d * d * 2); ALLOC(w.w_proj8, (size_t)d * 4 * d * 2);
        }
        ALLOC(w.b_in, 3 * d * 4); ALLOC(w.b_out, d * 4); ALLOC(w.b_fc, 4 * d * 4); ALLOC(w.b_proj, d * 4);
        ALLOC(w.ln1_g, d * 4); ALLOC(w.ln1_b, d * 4); ALLOC(w.ln2_g, d * 4); ALLOC(w.ln2_b, d * 4);
    }
    return MUDPT_OK;
}

// Bytes of activations + scratch per token row of a tower (what alloc_tower_acts takes per row; sizes the CoCoOp chunk).
static size_t tower_bytes_per_row(const Tower& t) {
    const size_t d = t.d, sp = 2;  // low halves counted always (upper bound)
    const size_t per_layer = d * 4 * 2 + d * 3 * 2 + d * 2 + d * 4 * 2 + 16 + (size_t)t.heads * 4 * 2;
    const size_t shared = d * 2 * sp * 2 + d * 4 * 2 * sp + d * 4 + d * 2 + d * 2 + d * 3 * 2 + d * 4 + (size_t)t.heads * 4 * 2 + d * 3 * 4;
    return per_layer * t.layers + shared;
}

// Activations saved for the backward + scratch, for max_seq sequences of L rows.  The vision tower's are made at create; the
// text tower's when the class prompts (and with them its trimmed length) are known -- and again if those change.
static int alloc_tower_acts(mudpt_model* m, Tower& t, int L, int max_seq) {
    for (void* p : t.act_allocs) (void)hipFree(p);
    t.act_allocs.clear();
#define ALLOC_T(ptr, bytes)                                                      \
    do {                                                                         \
        void* _p = nullptr;                                                      \
        HIP_TRY(hipMalloc(&_p, (size_t)(bytes) ? (size_t)(bytes) : 16));         \
        t.act_allocs.push_back(_p);                                              \
        *(void**)&(ptr) = _p;                                                    \
    } while (0)
    const int d = t.d, heads = t.heads;
    t.L = L; t.max_seq = max_seq; t.lay = nullptr;  // text tower: bind_text_layout follows
    t.Lp = attn_padded_len(L);
    const size_t M = (size_t)max_seq * L;
    for (int i = 0; i < t.layers; ++i) {
        BlockAct& a = t.a[i];
        ALLOC_T(a.x_in, M * d * 4); ALLOC_T(a.x_mid, M * d * 4);
        ALLOC_T(a.mean1, M * 4); ALLOC_T(a.rstd1, M * 4); ALLOC_T(a.mean2, M * 4); ALLOC_T(a.rstd2, M * 4);
        ALLOC_T(a.qkv, M * 3 * d * 2); ALLOC_T(a.attn, M * d * 2); ALLOC_T(a.u, M * 4 * d * 2);
        ALLOC_T(a.lse, (size_t)max_seq * heads * t.Lp * 4);
    }
    ALLOC_T(t.h, M * d * 2); ALLOC_T(t.g, M * 4 * d * 2);
    if (t.may_split) {  // the low halves of the split operands: the row length of their T counterparts in bytes, whatever their form
        ALLOC_T(t.h_lo, M * d * 2); ALLOC_T(t.g_lo, M * 4 * d * 2); ALLOC_T(t.attn_lo, M * d * 2);
    }
    ALLOC_T(t.dx, M * d * 4); ALLOC_T(t.dx_lp, M * d * 2);
    ALLOC_T(t.dattn, M * d * 2); ALLOC_T(t.dqkv, M * 3 * d * 2);
    ALLOC_T(t.delta, (size_t)max_seq * heads * t.Lp * 4);
    ALLOC_T(t.upd, M * d * 4);
    if (t.may_split && m->exact) ALLOC_T(t.qkv32, M * 3 * d * 4);
    const size_t S = (size_t)max_seq;
    ALLOC_T(t.xin_sel, S * d * 4); ALLOC_T(t.xmid_sel, S * d * 4); ALLOC_T(t.xout_sel, S * d * 4);
    ALLOC_T(t.attn_sel, S * d * 2); ALLOC_T(t.h_sel, S * d * 2); ALLOC_T(t.u_sel, S * 4 * d * 2); ALLOC_T(t.g_sel, S * 4 * d * 2); ALLOC_T(t.dattn_sel, S * d * 2);
    if (t.may_split) { ALLOC_T(t.attn_sel_lo, S * d * 2); ALLOC_T(t.h_sel_lo, S * d * 2); ALLOC_T(t.g_sel_lo, S * 4 * d * 2); }
    ALLOC_T(t.dsel, S * d * 4); ALLOC_T(t.dsel_lp, S * d * 2);
    ALLOC_T(t.q_sel, S * d * 2); ALLOC_T(t.dq_sel, S * d * 2); ALLOC_T(t.dqx_sel, S * d * 2); ALLOC_T(t.lse_sel, S * heads * 4);
    t.head_n = t.n;
    ALLOC_T(t.hd_dqkv, S * t.head_n * 3 * d * 2); ALLOC_T(t.hd_h, S * t.head_n * d * 2);
#undef ALLOC_T
    return MUDPT_OK;
}

static void expect_block_keys(mudpt_model* m, const std::string& prefix, int layers) {
    static const char* names[] = {"ln_1.weight", "ln_1.bias", "attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight",
                                  "attn.out_proj.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight", "mlp.c_fc.bias",
                                  "mlp.c_proj.weight", "mlp.c_proj.bias"};
    for (int i = 0; i < layers; ++i)
        for (const char* n : names) m->missing.push_back(prefix + ".resblocks." + std::to_string(i) + "." + n);
}

static int n_patches(const mudpt_config& c) { return (c.image_size / c.patch) * (c.image_size / c.patch); }  // per image
static int patch_k0(const mudpt_config& c) { return (3 * c.patch * c.patch + 63) / 64 * 64; }  // conv-as-GEMM K, zero-padded to the GEMM's granularity (ViT-L/14: 588 -> 640)

extern "C" int mudpt_abi_version(void) { return MUDPT_ABI_VERSION; }
extern "C" const char* mudpt_last_error(void) { return get_error(); }

// Fills a fresh model; on an error the caller (create_model) destroys it
static int create_impl(const mudpt_config* c, const mudpt_prompt_shape* ps, mudpt_model* m, bool frozen, bool resnet) {
    ARG_CHECK(c->dtype == MUDPT_BF16 || c->dtype == MUDPT_F16 || c->dtype == MUDPT_F32, "create: dtype must be MUDPT_BF16, MUDPT_F16 or MUDPT_F32");
    ARG_CHECK(c->variant >= MUDPT_VARIANT_MUDPT && c->variant <= MUDPT_VARIANT_UUMUDPT, "create: unknown variant %d", c->variant);
    m->cocoop = c->variant == MUDPT_VARIANT_COCOOP;
    m->csc = c->variant == MUDPT_VARIANT_COOP_CSC;
    m->coop = c->variant == MUDPT_VARIANT_COOP || m->csc;
    m->vpt = c->variant == MUDPT_VARIANT_VPT; m->mpt = c->variant == MUDPT_VARIANT_MPT; m->indep = m->vpt || m->mpt;
    m->uumudpt = c->variant == MUDPT_VARIANT_UUMUDPT;
    m->umudpt = c->variant == MUDPT_VARIANT_UMUDPT || m->uumudpt;
    m->frozen = frozen;  // mudpt_create_frozen: the caller passed variant MuDPT with n_ctx 0, depth 1 -- no prompt row anywhere
    const bool vanilla = m->cocoop || m->coop || frozen;  // the vanilla CLIP image encoder, forward only (no prompt rows, no deep prompts)
    ARG_CHECK(vanilla || m->indep || c->depth > 0, "PROMPT_DEPTH should be > 0");  // trainers/mudpt.py:52
    ARG_CHECK((m->indep || frozen || c->n_ctx > 0) && c->n_cls > 0 && c->max_batch > 0, "create: n_ctx, n_cls, max_batch must be positive");
    ARG_CHECK(c->patch > 0 && c->image_size % c->patch == 0, "create: image_size %d / patch %d unsupported", c->image_size, c->patch);
    ARG_CHECK(c->v_width == c->v_heads * 64 && c->t_width == c->t_heads * 64, "create: head dim must be 64");
    ARG_CHECK(c->v_width % 64 == 0 && c->t_width % 64 == 0 && c->v_width <= 1024 && c->t_width <= 1024, "create: widths must be multiples of 64, <= 1024");
    ARG_CHECK(!m->uumudpt || c->embed_dim == c->t_width, "create (UUMuDPT): embed_dim %d must equal t_width %d (visual_ctx_text_proj's output is added to "
              "deep_prompts, trainers/uumudpt.py:224)", c->embed_dim, c->t_width);
    ARG_CHECK(resnet || c->embed_dim == c->t_width, "create: embed_dim must equal t_width (visual_ctx_deep_projections output is added to text prompts)");  // a ResNet handle has no prompt: RN50 is 1024 / 512
    ARG_CHECK(m->indep || 1 + c->n_ctx < c->ctx_len, "create: n_ctx too large for ctx_len");
    if (m->umudpt) { if (int r = pg_check_shape(m->uumudpt ? "create (UUMuDPT)" : "create (UMuDPT)", c->depth, c->n_ctx, c->t_width, c->v_width)) return r; }
    if (m->uumudpt && c->depth > 1) { if (int r = pg_check_shape("create (UUMuDPT, the vision tower's generator)", c->depth - 1, c->n_ctx, c->v_width, c->embed_dim)) return r; }
    // prompt rows and deep-prompt layers per tower (Tower::n, Tower::D1)
    int nv = vanilla ? 0 : c->n_ctx, D1v = vanilla ? 0 : c->depth - 1, nt = c->n_ctx, D1t = vanilla ? 0 : c->depth - 1;
    if (m->indep) {
        const char* T = m->vpt ? "VPT" : "MPT";
        ARG_CHECK(ps->t_n_ctx >= 0 && ps->v_n_ctx >= 0, "create_ex: TRAINER.%s.DEEP_TEXT_N_CTX %d / DEEP_VISUAL_N_CTX %d must be >= 0", T, ps->t_n_ctx, ps->v_n_ctx);
        // the vision prompt exists only for 0 < VISUAL_PROMPT_DEPTH <= 12, whatever the layer count (clip/model.py:459)
        const bool vprompt = ps->v_n_ctx > 0 && ps->v_depth > 0 && ps->v_depth <= 12;
        if (m->vpt) {
            ARG_CHECK(vprompt, "create_ex: VPT without a vision prompt (TRAINER.VPT.DEEP_VISUAL_N_CTX %d, TRAINER.VPT.VISUAL_PROMPT_DEPTH %d: "
                      "needs > 0 and 1..12) has nothing to train", ps->v_n_ctx, ps->v_depth);
            ARG_CHECK(!(ps->t_n_ctx > 0 && ps->t_depth > 1), "create_ex: VPT with text deep prompts (TRAINER.VPT.DEEP_TEXT_N_CTX %d, "
                      "TRAINER.VPT.TEXT_PROMPT_DEPTH %d) is not supported: use MPT", ps->t_n_ctx, ps->t_depth);
        } else {
            ARG_CHECK(ps->t_n_ctx >= 1, "create_ex: MPT needs TRAINER.MPT.DEEP_TEXT_N_CTX >= 1 (got %d)", ps->t_n_ctx);
            ARG_CHECK(1 + ps->t_n_ctx < c->ctx_len, "create_ex: TRAINER.MPT.DEEP_TEXT_N_CTX %d too large for ctx_len %d", ps->t_n_ctx, c->ctx_len);
        }
        nv = vprompt ? ps->v_n_ctx : 0;
        D1v = vprompt ? std::min(ps->v_depth, c->v_layers) - 1 : 0;  // blocks 1 <= i < depth own a visual_ctx (clip/model.py:404-416)
        nt = m->mpt ? ps->t_n_ctx : 0;
        D1t = m->mpt ? std::max(0, std::min(ps->t_depth, c->t_layers) - 1) : 0;  // no cap on the text depth (clip/model.py:752-770)
    }
    const int P = n_patches(*c);
    const int Lv = 1 + P + nv;  // CoCoOp's / CoOp's image encoder is the vanilla ViT (trainers/cocoop.py:38, coop.py:37, clip/model.py:443-496)
    ARG_CHECK(Lv <= 4096 && c->ctx_len <= 4096, "create: sequence length %d/%d exceeds the attention limit (4096)", Lv, c->ctx_len);

    m->cfg = *c;
    // MUDPT_F32 (the parity mode): the kernels' operand type is fp16.  Text tower: every forward GEMM operand a 22-bit
    // (hi, lo) pair and the attention forward in fp32 -- each of its rounding sites alone costs 2.5e-3 on the logits at logit scale 100.
    // Vision tower: every forward GEMM operand (and the pixels) hi + an e4m3 remainder contracted on the fp8 matrix pipe, attention in
    // fp16.  Knobs vis_lo / vis_exact_attn / vis_sites / txt_sites select the other points of the ablation (vis_lo = 1, vis_exact_attn = 1:
    // round 3's "exact" mode).  MUDPT_F16 splits the text tower's GEMM operands only (the round-2 mode, kept as it was).
    m->exact = c->dtype == MUDPT_F32;
    m->dtype = m->exact ? (int)MUDPT_F16 : c->dtype;
    m->vis.may_split = m->exact;
    m->txt.may_split = m->dtype == MUDPT_F16;
    m->vis.split = m->exact ? LO_F8 : LO_NONE;
    m->txt.split = m->txt.may_split ? LO_F16 : LO_NONE;
    m->txt.exact_attn = m->exact;
    // the gradient of the residual stream in T: bf16 mode, and the parity mode (its bound is on the LOGITS; its backward is the fp16 mode's
    // with fp16 activation gradients, as the reference's own fp16 model has them: gradient errors +30 %, -0.9 ms per step; knob lp_grad = 0)
    m->lp_grad = (c->dtype == MUDPT_BF16 || c->dtype == MUDPT_F32);
    m->lp_upd = (c->dtype == MUDPT_BF16);
    m->gelu_q8 = (c->dtype == MUDPT_BF16);
    m->ct = c->n_cls;
    if (vanilla || m->indep) m->cfg.depth = 1;  // no MuDPT deep prompts
    if (m->indep) m->cfg.n_ctx = nt;            // the text prompt rows (mudpt_set_class_prompts)
    m->vis.n = nv; m->vis.D1 = D1v; m->txt.n = nt; m->txt.D1 = D1t;
    const int dv = c->v_width, dt = c->t_width, e = c->embed_dim, n = m->cfg.n_ctx, D1 = m->cfg.depth - 1, B = c->max_batch, C = c->n_cls;
    const int TS = m->cocoop ? B * C : C;  // text sequences per step: one per (image, class) pair in CoCoOp (trainers/cocoop.py:187-194)
    if (int r = alloc_tower_weights(m, m->vis, dv, c->v_layers, c->v_heads, false, Lv - nv, m->exact)) return r;  // e4m3 weight copies: vision tower of the parity mode
    if (int r = alloc_tower_acts(m, m->vis, Lv, B)) return r;
    // the text tower's activations are sized by mudpt_set_class_prompts: its trimmed length (max(eot) + 1 of ctx_len positions) and, for
    // CoCoOp, the number of images whose B * C prompts fit the memory budget at once are only known there
    if (int r = alloc_tower_weights(m, m->txt, dt, c->t_layers, c->t_heads, true, 1, false)) return r;
    const int K0 = patch_k0(*c);
    ALLOC(m->conv_w, (size_t)dv * K0 * 2);
    if (m->exact) { ALLOC(m->conv_w8, (size_t)dv * K0 * 2); ALLOC(m->patches_lo, (size_t)B * P * K0 * 2); }  // split pixels (vision tower's site 4)
    ALLOC(m->cls, dv * 4); ALLOC(m->vpos, (size_t)(1 + P) * dv * 4);
    ALLOC(m->ln_pre_g, dv * 4); ALLOC(m->ln_pre_b, dv * 4); ALLOC(m->ln_post_g, dv * 4); ALLOC(m->ln_post_b, dv * 4);
    ALLOC(m->vproj, (size_t)dv * e * 4);
    ALLOC(m->patches, (size_t)B * P * K0 * 2);
    ALLOC(m->xpre, (size_t)B * Lv * dv * 4); ALLOC(m->pre_mean, (size_t)B * Lv * 4); ALLOC(m->pre_rstd, (size_t)B * Lv * 4);
    ALLOC(m->f_ln, (size_t)B * dv * 4); ALLOC(m->post_mean, B * 4); ALLOC(m->post_rstd, B * 4); ALLOC(m->df_ln, (size_t)B * dv * 4);
    ALLOC(m->cls_rows, B * 4); ALLOC(m->vprompt_rows, (size_t)B * nv * 4);
    ALLOC(m->tpos, (size_t)c->ctx_len * dt * 4); ALLOC(m->ln_fin_g, dt * 4); ALLOC(m->ln_fin_b, dt * 4);
    ALLOC(m->tproj, (size_t)dt * e * 4);
    ALLOC(m->emb_pos, frozen ? 0 : (size_t)C * c->ctx_len * dt * 4);  // frozen: embedded on the device, template by template
    ALLOC(m->lay.eot_rows, TS * 4); ALLOC(m->lay.eot_local, TS * 4); ALLOC(m->lay.perm, C * 4);
    ALLOC(m->txt_sorted, (size_t)C * e * 4); ALLOC(m->dtxt_sorted, (size_t)C * e * 4);
    ALLOC(m->t_ln, (size_t)TS * dt * 4); ALLOC(m->fin_mean, TS * 4); ALLOC(m->fin_rstd, TS * 4); ALLOC(m->dt_ln, (size_t)TS * dt * 4);
    const size_t dn = (size_t)(D1 > 0 ? D1 : 1) * n;
    ALLOC(m->shared, (size_t)n * dv * 4); ALLOC(m->t2v, dn * dv * 4); ALLOC(m->v2t, dn * e * 4);
    ALLOC(m->vis_deep, dn * dv * 4); ALLOC(m->txt_deep, dn * dt * 4);
    ALLOC(m->vsplice, (size_t)B * (D1v > 0 ? D1v : 1) * nv * dv * 4);
    ALLOC(m->d_vis_deep, dn * dv * 4); ALLOC(m->d_txt_deep, dn * dt * 4); ALLOC(m->d_vprompt0, (size_t)n * dv * 4);
    ALLOC(m->img_f, (size_t)B * e * 4); ALLOC(m->txt_f, (size_t)TS * e * 4); ALLOC(m->img_n, (size_t)B * e * 4); ALLOC(m->txt_n, (size_t)TS * e * 4);
    ALLOC(m->img_inv, B * 4); ALLOC(m->txt_inv, TS * 4);
    ALLOC(m->logits, (size_t)B * C * 4); ALLOC(m->dlogits, (size_t)B * C * 4); ALLOC(m->row_loss, B * 4);
    if (!resnet) ALLOC(m->dimg, (size_t)B * e * 4);  // a ResNet tower is frozen and prompt-free: head_train asks for no image gradient
    ALLOC(m->dtxt, (size_t)TS * e * 4); ALLOC(m->loss, 16);
    if (m->cocoop) {
        m->hid = e / 16;
        ALLOC(m->mn_hid, (size_t)B * m->hid * 4); ALLOC(m->mn_dhid, (size_t)B * m->hid * 4);
        ALLOC(m->mn_bias, (size_t)B * dt * 4); ALLOC(m->mn_dbias, (size_t)B * dt * 4);
    }
    if (m->coop) ALLOC(m->coop_pos, (size_t)C * n * 4);
    if (m->umudpt) {
        const size_t R = (size_t)c->depth * n;
        size_t ws = 0;
        (void)pg_carve(nullptr, c->depth, n, dt, &ws);
        ALLOC(m->pg_G, R * dv * 4); ALLOC(m->pg_dG, R * dv * 4); ALLOC(m->pg_dX, R * dt * 4); ALLOC(m->pg_ws, ws * 4);
        m->pg_w = pg_carve(m->pg_ws, c->depth, n, dt, nullptr);
    }
    if (m->uumudpt && D1 > 0) {
        size_t ws = 0;
        (void)pg_carve(nullptr, D1, n, dv, &ws);
        ALLOC(m->pg2_T, (size_t)D1 * n * e * 4); ALLOC(m->pg2_ws, ws * 4);
        m->pg2_w = pg_carve(m->pg2_ws, D1, n, dv, nullptr);
    }
    if (frozen) ALLOC(m->ens_acc, (size_t)C * e * 4);
    ALLOC(m->gemm_scratch, mudpt_model::kScratchElems * 4); ALLOC(m->gemm_scratch2, mudpt_model::kScratchElems * 4);
    HIP_TRY(hipStreamCreateWithFlags(&m->s2, hipStreamNonBlocking));
    for (hipEvent_t* e : {&m->ev_fork, &m->ev_join, &m->ev_fork_b, &m->ev_join_b}) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
    // row index tables
    std::vector<int> cr(B), pr((size_t)B * nv);
    for (int b = 0; b < B; ++b) {
        cr[b] = b * Lv;
        for (int i = 0; i < nv; ++i) pr[(size_t)b * nv + i] = b * Lv + (Lv - nv) + i;
    }
    HIP_TRY(hipMemcpy(m->cls_rows, cr.data(), cr.size() * 4, hipMemcpyHostToDevice));
    m->vis.tail_rows = m->cls_rows;
    m->vis.head_rows = nv > 0 ? m->vprompt_rows : nullptr;
    ALLOC(m->tprompt_rows, (size_t)TS * nt * 4);
    m->txt.head_rows = nt > 0 ? m->tprompt_rows : nullptr;  // ctx rows of every prompt; filled by mudpt_set_class_prompts, which binds the EOT rows too
    HIP_TRY(hipMemcpy(m->vprompt_rows, pr.data(), pr.size() * 4, hipMemcpyHostToDevice));

    if (!frozen) build_trainables(m);  // a frozen handle has none: mudpt_param_count / _numel report 0
    ALLOC(m->momentum, m->total * 4);

    // frozen weights the path needs before it may run
    for (const char* k : {"visual.conv1.weight", "visual.class_embedding", "visual.positional_embedding", "visual.ln_pre.weight",
                          "visual.ln_pre.bias", "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj", "positional_embedding",
                          "ln_final.weight", "ln_final.bias", "text_projection", "logit_scale"})
        m->missing.push_back(k);
    expect_block_keys(m, "visual.transformer", c->v_layers);
    expect_block_keys(m, "transformer", c->t_layers);
    if (frozen) m->missing.push_back("token_embedding.weight");
    return MUDPT_OK;
}

static int resnet_setup(mudpt_model* m, int image_size, const mudpt_resnet_shape& shape);
// rn: a ResNet image tower is set up behind the (then block-less) ViT fields, for images of rn_image_size
static int create_model(const mudpt_config* c, const mudpt_prompt_shape* ps, mudpt_model** out, bool frozen = false, const mudpt_resnet_shape* rn = nullptr,
                        int rn_image_size = 0) {
    mudpt_model* m = new mudpt_model();
    int rc = create_impl(c, ps, m, frozen, rn != nullptr);
    if (!rc && rn) rc = resnet_setup(m, rn_image_size, *rn);
    if (rc) { mudpt_destroy(m); return rc; }
    *out = m;
    return MUDPT_OK;
}

extern "C" int mudpt_create(const mudpt_config* c, mudpt_model** out) {
    ARG_CHECK(c && out, "create: null argument");
    ARG_CHECK(c->variant != MUDPT_VARIANT_VPT && c->variant != MUDPT_VARIANT_MPT,
              "create: variant %d (VPT / MPT) needs the per-tower prompt shape: use mudpt_create_ex", c->variant);
    return create_model(c, nullptr, out);
}

extern "C" int mudpt_create_ex(const mudpt_config* c, const mudpt_prompt_shape* ps, mudpt_model** out) {
    ARG_CHECK(c && out, "create_ex: null argument");
    // whether a shape must come with the call is decided before a model exists; the model's own flags are derived in create_impl
    const bool per_tower = c->variant == MUDPT_VARIANT_VPT || c->variant == MUDPT_VARIANT_MPT;
    ARG_CHECK(!per_tower || ps, "create_ex: variant %d (VPT / MPT) needs a mudpt_prompt_shape", c->variant);
    ARG_CHECK(per_tower || !ps, "create_ex: a mudpt_prompt_shape is for VPT / MPT only (variant %d: pass NULL)", c->variant);
    return create_model(c, ps, out);
}

// Frozen CLIP (trainers/zsclip.py): variant, n_ctx and depth of the caller's config are not read -- the handle is built as a tower pair without
// a single prompt row, which is what those three fields would describe
extern "C" int mudpt_create_frozen(const mudpt_config* c, mudpt_model** out) {
    ARG_CHECK(c && out, "create_frozen: null argument");
    mudpt_config f = *c;
    f.variant = MUDPT_VARIANT_MUDPT; f.n_ctx = 0; f.depth = 1;
    return create_model(&f, nullptr, out, true);
}

// ---- frozen CLIP with the ResNet image tower (clip/model.py:17-161, 686-694, 890-897) ----
static int round_up64(int v) { return (v + 63) / 64 * 64; }
// fp64 -> T with ONE rounding (a detour over fp32 rounds twice): fp16 by the compiler's conversion, bf16 over an fp32 rounded to odd
static inline uint16_t f64_to_lp(int dtype, double d) {
    if (dtype == DT_F16) {
        const _Float16 h = (_Float16)d;
        uint16_t u;
        memcpy(&u, &h, 2);
        return u;
    }
    float f = (float)d;
    if ((double)f != d && std::isfinite(f)) {  // inexact: keep the truncated magnitude and set the sticky bit
        uint32_t u;
        memcpy(&u, &f, 4);
        const bool above = std::fabs((double)f) > std::fabs(d);
        if (!(u & 1u)) u = above ? u - 1 : u + 1;
        memcpy(&f, &u, 4);
    }
    return f32_to_bf16(f);
}
// mudpt_conv_pack (include/mudpt.h): the one statement of the BatchNorm folding and of the packed weight layout
static void conv_pack(int dtype, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int cout, int cin, int k, int ldk,
                      uint16_t* w_out, float* bias_out) {
    for (int o = 0; o < cout; ++o) {
        const double scale = (double)gamma[o] / std::sqrt((double)var[o] + 1e-5);
        bias_out[o] = (float)((double)beta[o] - (double)mean[o] * scale);
        uint16_t* row = w_out + (size_t)o * ldk;
        for (int t = 0; t < k * k; ++t)
            for (int c = 0; c < cin; ++c) row[t * cin + c] = f64_to_lp(dtype, (double)w[((size_t)o * cin + c) * k * k + t] * scale);
        for (int j = k * k * cin; j < ldk; ++j) row[j] = 0;
    }
}

// The tower's convolutions in the reference's module order, its device weights and its activations for max_batch images
static int resnet_setup(mudpt_model* m, int S, const mudpt_resnet_shape& shape) {
    Resnet* r = new Resnet();
    m->rn = r;
    r->shape = shape; r->S = S; r->C = 32 * shape.width; r->L = (S / 32) * (S / 32) + 1;
    m->cfg.image_size = S;
    const int w = shape.width, B = m->cfg.max_batch, e = m->cfg.embed_dim, C = r->C, L = r->L;
    size_t act = 0, rows = 0, acc = 0;  // elements per image
    // a convolution on an H x H input whose output a 1 x 1 convolution (or nothing) reads next; returns its index
    auto conv = [&](const std::string& cname, const std::string& bname, int cin, int cout, int k, bool feeds_1x1, int H, int stride) {
        RnConv c;
        c.conv = cname; c.bn = bname; c.cin = cin; c.cout = cout; c.k = k;
        c.ldk = round_up64(k * k * cin);
        c.np = feeds_1x1 ? round_up64(cout) : cout;
        const size_t Ho = (size_t)((H - 1) / stride + 1), px = Ho * Ho;
        act = std::max(act, px * c.np); acc = std::max(acc, px * c.np);
        if (k == 3) rows = std::max(rows, px * c.ldk);
        r->convs.push_back(c);
        return (int)r->convs.size() - 1;
    };
    int H = S / 2;
    conv("visual.conv1", "visual.bn1", 3, w / 2, 3, false, S, 2);
    conv("visual.conv2", "visual.bn2", w / 2, w / 2, 3, false, H, 1);
    conv("visual.conv3", "visual.bn3", w / 2, w, 3, true, H, 1);
    H /= 2;  // AvgPool2d(2)
    int inplanes = w;
    const int counts[4] = {shape.layers1, shape.layers2, shape.layers3, shape.layers4};
    for (int st = 0; st < 4; ++st) {
        const int planes = w << st;
        for (int i = 0; i < counts[st]; ++i) {
            const std::string p = "visual.layer" + std::to_string(st + 1) + "." + std::to_string(i) + ".";
            RnBlock b;
            b.stride = (st > 0 && i == 0) ? 2 : 1;
            const int Ho = H / b.stride;
            b.conv1 = conv(p + "conv1", p + "bn1", inplanes, planes, 1, false, H, 1);
            b.conv2 = conv(p + "conv2", p + "bn2", planes, planes, 3, true, H, 1);
            b.conv3 = conv(p + "conv3", p + "bn3", planes, 4 * planes, 1, true, Ho, 1);
            if (b.stride > 1 || inplanes != 4 * planes) b.down = conv(p + "downsample.0", p + "downsample.1", inplanes, 4 * planes, 1, true, Ho, 1);
            r->blocks.push_back(b);
            inplanes = 4 * planes;
            H = Ho;
        }
    }
    for (RnConv& c : r->convs) { ALLOC(c.w_dev, (size_t)c.np * c.ldk * 2); ALLOC(c.b_dev, (size_t)c.np * 4); }
    ALLOC(r->pos, (size_t)L * C * 4); ALLOC(r->b_q, (size_t)C * 4); ALLOC(r->b_kv, (size_t)2 * C * 4); ALLOC(r->b_c, (size_t)e * 4);
    ALLOC(r->w_q, (size_t)C * C * 2); ALLOC(r->w_kv, (size_t)2 * C * C * 2); ALLOC(r->w_c, (size_t)e * C * 2);
    for (void*& a : r->act) ALLOC(a, (size_t)B * act * 2);
    ALLOC(r->rows, (size_t)B * rows * 2); ALLOC(r->acc, (size_t)B * acc * 4);
    ALLOC(r->tok, (size_t)B * L * C * 2); ALLOC(r->ao, (size_t)B * C * 2);
    ALLOC(r->q, (size_t)B * C * 4); ALLOC(r->kv, (size_t)B * L * 2 * C * 4);
    // the keys the tower needs before it may run, instead of the ViT's
    m->missing.erase(std::remove_if(m->missing.begin(), m->missing.end(), [](const std::string& k) { return k.rfind("visual.", 0) == 0; }), m->missing.end());
    for (const RnConv& c : r->convs) {
        m->missing.push_back(c.conv + ".weight");
        for (const char* n : {".weight", ".bias", ".running_mean", ".running_var"}) m->missing.push_back(c.bn + n);
    }
    m->missing.push_back("visual.attnpool.positional_embedding");
    for (const char* n : {"q_proj", "k_proj", "v_proj", "c_proj"})
        for (const char* x : {".weight", ".bias"}) m->missing.push_back(std::string("visual.attnpool.") + n + x);
    return MUDPT_OK;
}

// What both ResNet entry points refuse, each before any device call (`fn` opens the message)
static int resnet_check(const char* fn, const mudpt_config* c, const mudpt_resnet_shape* rn) {
    ARG_CHECK(c->dtype != MUDPT_F32, "%s: dtype MUDPT_F32: ResNet towers run in bf16 / fp16; the parity mode is not built for them", fn);
    ARG_CHECK(c->image_size >= 32 && c->image_size % 32 == 0, "%s: image_size %d must be a positive multiple of 32 (the tower divides it by 32)", fn, c->image_size);
    ARG_CHECK(rn->layers1 >= 1 && rn->layers2 >= 1 && rn->layers3 >= 1 && rn->layers4 >= 1, "%s: layers (%d, %d, %d, %d): every stage needs at least one block", fn,
              rn->layers1, rn->layers2, rn->layers3, rn->layers4);
    ARG_CHECK(rn->width >= 32 && rn->width % 32 == 0, "%s: width %d must be a positive multiple of 32: the stem has width / 2 channels and the GEMM needs N %% 16 == 0 "
              "(RN50x4, width 80, has a 40-channel stem and is not built)", fn, rn->width);
    ARG_CHECK(rn->heads >= 1 && (32 * rn->width) % rn->heads == 0, "%s: heads %d must be >= 1 and divide 32 * width = %d", fn, rn->heads, 32 * rn->width);
    ARG_CHECK(32 * rn->width / rn->heads == 64, "%s: heads %d gives a head dimension of %d; the attention pool runs 64 (heads = 32 * width / 64, clip/model.py:687)", fn,
              rn->heads, 32 * rn->width / rn->heads);
    ARG_CHECK(c->embed_dim >= 16 && c->embed_dim % 16 == 0, "%s: embed_dim %d must be a positive multiple of 16 (c_proj's GEMM N)", fn, c->embed_dim);
    return MUDPT_OK;
}
// behind the tower the handle is a ViT handle's; its ViT fields describe one 32 x 32 patch and no block, and are never run
static mudpt_config resnet_vit_stub(const mudpt_config& c) {
    mudpt_config f = c;
    f.image_size = 32; f.patch = 32; f.v_width = 64; f.v_layers = 0; f.v_heads = 1;
    return f;
}

extern "C" int mudpt_create_frozen_resnet(const mudpt_config* c, const mudpt_resnet_shape* rn, mudpt_model** out) {
    ARG_CHECK(c && rn && out, "create_frozen_resnet: null argument");
    if (int rc = resnet_check("create_frozen_resnet", c, rn)) return rc;
    mudpt_config f = resnet_vit_stub(*c);  // ... mudpt_create_frozen's
    f.variant = MUDPT_VARIANT_MUDPT; f.n_ctx = 0; f.depth = 1;
    return create_model(&f, nullptr, out, true, rn, c->image_size);
}

// CoOp / CoCoOp with the ResNet image tower (trainers/coop.py:212-226, cocoop.py:178-198: the image encoder is frozen and prompt-free, so the
// tower runs forward only where the vanilla ViT would).  The other variants put trainable prompts into a ViT's token sequence
extern "C" int mudpt_create_resnet(const mudpt_config* c, const mudpt_resnet_shape* rn, mudpt_model** out) {
    ARG_CHECK(c && rn && out, "create_resnet: null argument");
    static const char* names[] = {"MuDPT", "CoCoOp", "CoOp", "CoOp (CSC)", "VPT", "MPT", "UMuDPT", "UUMuDPT"};
    ARG_CHECK(c->variant >= MUDPT_VARIANT_MUDPT && c->variant <= MUDPT_VARIANT_UUMUDPT, "create_resnet: unknown variant %d", c->variant);
    ARG_CHECK(c->variant == MUDPT_VARIANT_COOP || c->variant == MUDPT_VARIANT_COOP_CSC || c->variant == MUDPT_VARIANT_COCOOP,
              "create_resnet: variant %d (%s): its prompts live inside a ViT; a ResNet image tower serves CoOp, CoOp with CSC and CoCoOp", c->variant, names[c->variant]);
    if (int rc = resnet_check("create_resnet", c, rn)) return rc;
    const mudpt_config f = resnet_vit_stub(*c);
    return create_model(&f, nullptr, out, false, rn, c->image_size);
}

// include/mudpt.h: which launches resnet_conv makes from the next forward on
extern "C" int mudpt_resnet_conv_path(mudpt_model* m, int32_t path) {
    ARG_CHECK(m, "resnet_conv_path: null model");
    ARG_CHECK(m->rn, "resnet_conv_path: this handle has no ResNet image tower (mudpt_create_frozen_resnet, mudpt_create_resnet make one)");
    ARG_CHECK(path == 0 || path == 1, "resnet_conv_path: path %d (0: im2col + GEMM + bias_act, 1: mudpt_conv2d)", path);
    m->rn->conv_path = path;
    return MUDPT_OK;
}

// every entry point that trains, takes embedded class prompts or shards the classes
#define NOT_FROZEN(m, what) ARG_CHECK(!((m) && (m)->frozen), "%s: a frozen handle (mudpt_create_frozen) has no parameters, class-prompt embeddings or class shards", what)

extern "C" int mudpt_destroy(mudpt_model* m) {
    if (!m) return MUDPT_OK;
    if (m->tok_table) (void)hipFree(m->tok_table);
    delete m->rn;  // its device buffers are in m->allocs
    if (m->tmpl_tables) (void)hipFree(m->tmpl_tables);
    for (void* p : m->allocs) (void)hipFree(p);
    for (Tower* t : {&m->vis, &m->txt})
        for (void* p : t->act_allocs) (void)hipFree(p);
    for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : {m->ev_fork, m->ev_join, m->ev_fork_b, m->ev_join_b})
        if (e) (void)hipEventDestroy(e);
    if (m->s2) (void)hipStreamDestroy(m->s2);
    delete m;
    return MUDPT_OK;
}

// ---- weight ingestion -----------------------------------------------------------------------------------
static int upload_f32(float* dst, const float* src, size_t n) {
    HIP_TRY(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice));
    return MUDPT_OK;
}
// W [rows, cols] fp32 host -> T device, plain and (optionally) transposed copies
static int upload_lp(int dtype, void* dst, void* dst_t, const float* src, size_t rows, size_t cols) {
    std::vector<uint16_t> tmp(rows * cols);
    auto cv = [&](float f) { return dtype == DT_BF16 ? f32_to_bf16(f) : f32_to_f16(f); };
    for (size_t i = 0; i < rows * cols; ++i) tmp[i] = cv(src[i]);
    HIP_TRY(hipMemcpy(dst, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    if (dst_t) {
        for (size_t r = 0; r < rows; ++r)
            for (size_t c = 0; c < cols; ++c) tmp[c * rows + r] = cv(src[r * cols + c]);
        HIP_TRY(hipMemcpy(dst_t, tmp.data(), tmp.size() * 2, hipMemcpyHostToDevice));
    }
    return MUDPT_OK;
}

// W [rows, cols] fp32 host -> e4m3 device copy for the second pass of a LO_F8 split GEMM: rows of 2 * cols BYTES (the T copy's row length, so
// that byte offsets into W and W8 agree), the first cols of them W 2^shift in e4m3; *scale_e8m0 = the block scale 2^-shift for the MFMA
static int upload_e4m3(void* dst, int* scale_e8m0, const float* src, size_t rows, size_t cols) {
    float mx = 0.f;
    for (size_t i = 0; i < rows * cols; ++i) mx = std::max(mx, std::fabs(src[i]));
    int shift = 0;
    if (mx > 0.f && std::isfinite(mx)) {
        shift = (int)std::floor(std::log2(448.f / mx));
        while (std::ldexp(mx, shift) > 448.f) --shift;
        shift = std::max(-100, std::min(100, shift));
    }
    std::vector<uint8_t> tmp(rows * 2 * cols, 0);
    for (size_t r = 0; r < rows; ++r)
        for (size_t c = 0; c < cols; ++c) tmp[r * 2 * cols + c] = f32_to_e4m3(std::ldexp(src[r * cols + c], shift));
    HIP_TRY(hipMemcpy(dst, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    *scale_e8m0 = 127 - shift;
    return MUDPT_OK;
}

static int set_block_weight(mudpt_model* m, Tower& t, int layer, const std::string& name, const float* data, size_t numel) {
    ARG_CHECK(layer >= 0 && layer < t.layers, "set_weight: layer %d out of range", layer);
    BlockW& w = t.w[layer];
    const size_t d = t.d;
    struct F32 { const char* n; float* p; size_t sz; };
    const F32 f32s[] = {{"ln_1.weight", w.ln1_g, d}, {"ln_1.bias", w.ln1_b, d}, {"ln_2.weight", w.ln2_g, d}, {"ln_2.bias", w.ln2_b, d},
                        {"attn.in_proj_bias", w.b_in, 3 * d}, {"attn.out_proj.bias", w.b_out, d}, {"mlp.c_fc.bias", w.b_fc, 4 * d},
                        {"mlp.c_proj.bias", w.b_proj, d}};
    for (const F32& f : f32s)
        if (name == f.n) {
            ARG_CHECK(numel == f.sz, "set_weight: %s expects %zu elements, got %zu", f.n, f.sz, numel);
            return upload_f32(f.p, data, numel);
        }
    struct LP { const char* n; void* p; void* pt; void* p8; int* s8; size_t rows, cols; };
    const LP lps[] = {{"attn.in_proj_weight", w.w_in, w.w_in_t, w.w_in8, &w.s_in8, 3 * d, d}, {"attn.out_proj.weight", w.w_out, w.w_out_t, w.w_out8, &w.s_out8, d, d},
                      {"mlp.c_fc.weight", w.w_fc, w.w_fc_t, w.w_fc8, &w.s_fc8, 4 * d, d}, {"mlp.c_proj.weight", w.w_proj, w.w_proj_t, w.w_proj8, &w.s_proj8, d, 4 * d}};
    for (const LP& l : lps)
        if (name == l.n) {
            ARG_CHECK(numel == l.rows * l.cols, "set_weight: %s expects %zu elements, got %zu", l.n, l.rows * l.cols, numel);
            if (l.p8) { if (int rc = upload_e4m3(l.p8, l.s8, data, l.rows, l.cols)) return rc; }
            return upload_lp(m->dtype, l.p, l.pt, data, l.rows, l.cols);
        }
    set_error("set_weight: unknown block tensor '%s'", name.c_str());
    return MUDPT_ERR_ARG;
}

// A "visual.*" tensor of a ResNet handle.  Convolutions and BatchNorm statistics are kept on the host as they arrive and folded at the next
// forward (resnet_fold); the attention pool's tensors go to the device at once, its Linear weights in T
static int resnet_set_weight(mudpt_model* m, const std::string& k, const float* data, size_t numel) {
    Resnet& r = *m->rn;
    const size_t C = r.C, L = r.L, e = m->cfg.embed_dim;
    const char* key = k.c_str();
#define EXPECT(n) ARG_CHECK(numel == (size_t)(n), "set_weight: %s expects %zu elements, got %zu", key, (size_t)(n), numel)
    static const char* tracked = ".num_batches_tracked";
    if (k.size() > strlen(tracked) && k.compare(k.size() - strlen(tracked), strlen(tracked), tracked) == 0) return MUDPT_OK;  // BatchNorm's step counter: eval mode never reads it
    r.stale = true;
    static const char* bn_names[4] = {".weight", ".bias", ".running_mean", ".running_var"};
    for (RnConv& c : r.convs) {
        if (k == c.conv + ".weight") { EXPECT((size_t)c.cout * c.cin * c.k * c.k); c.w.assign(data, data + numel); return MUDPT_OK; }
        for (int i = 0; i < 4; ++i)
            if (k == c.bn + bn_names[i]) { EXPECT(c.cout); c.bnp[i].assign(data, data + numel); return MUDPT_OK; }
    }
    const std::string ap = "visual.attnpool.";
    if (k == ap + "positional_embedding") { EXPECT(L * C); return upload_f32(r.pos, data, numel); }
    if (k == ap + "q_proj.weight") { EXPECT(C * C); return upload_lp(m->dtype, r.w_q, nullptr, data, C, C); }
    if (k == ap + "k_proj.weight") { EXPECT(C * C); return upload_lp(m->dtype, r.w_kv, nullptr, data, C, C); }
    if (k == ap + "v_proj.weight") { EXPECT(C * C); return upload_lp(m->dtype, (char*)r.w_kv + C * C * 2, nullptr, data, C, C); }
    if (k == ap + "c_proj.weight") { EXPECT(e * C); return upload_lp(m->dtype, r.w_c, nullptr, data, e, C); }
    if (k == ap + "q_proj.bias") { EXPECT(C); return upload_f32(r.b_q, data, numel); }
    if (k == ap + "k_proj.bias") { EXPECT(C); return upload_f32(r.b_kv, data, numel); }
    if (k == ap + "v_proj.bias") { EXPECT(C); return upload_f32(r.b_kv + C, data, numel); }
    if (k == ap + "c_proj.bias") { EXPECT(e); return upload_f32(r.b_c, data, numel); }
#undef EXPECT
    set_error("set_weight: unknown key '%s' for a ResNet image tower with stages (%d, %d, %d, %d)", key, r.shape.layers1, r.shape.layers2, r.shape.layers3, r.shape.layers4);
    return MUDPT_ERR_ARG;
}

// BatchNorm folding + packing of every convolution, on the host in fp64, and the upload: at the first forward after a "visual.*" tensor
// arrived.  The stream is drained first: a forward in flight may still read the weights this overwrites
static int resnet_fold(mudpt_model* m, hipStream_t s) {
    Resnet& r = *m->rn;
    HIP_TRY(hipStreamSynchronize(s));
    std::vector<uint16_t> wp;
    std::vector<float> bp;
    for (const RnConv& c : r.convs) {
        wp.assign((size_t)c.np * c.ldk, 0);
        bp.assign(c.np, 0.f);
        conv_pack(m->dtype, c.w.data(), c.bnp[0].data(), c.bnp[1].data(), c.bnp[2].data(), c.bnp[3].data(), c.cout, c.cin, c.k, c.ldk, wp.data(), bp.data());
        HIP_TRY(hipMemcpy(c.w_dev, wp.data(), wp.size() * 2, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(c.b_dev, bp.data(), bp.size() * 4, hipMemcpyHostToDevice));
    }
    r.stale = false;
    return MUDPT_OK;
}

extern "C" int mudpt_set_weight(mudpt_model* m, const char* key, const float* data, size_t numel) {
    ARG_CHECK(m && key && data, "set_weight: null argument");
    m->cl_B = 0;  // a new weight ends a mudpt_forward_train in flight
    const mudpt_config& c = m->cfg;
    const std::string k(key);
    const size_t dv = c.v_width, dt = c.t_width, e = c.embed_dim;
    const size_t P = (size_t)n_patches(c);
    int rc = MUDPT_OK;
    auto blk = [&](const char* prefix, Tower& t) -> int {
        const std::string rest = k.substr(strlen(prefix));
        const size_t dot = rest.find('.');
        ARG_CHECK(dot != std::string::npos, "set_weight: malformed key %s", key);
        return set_block_weight(m, t, atoi(rest.substr(0, dot).c_str()), rest.substr(dot + 1), data, numel);
    };
#define EXPECT(n) ARG_CHECK(numel == (size_t)(n), "set_weight: %s expects %zu elements, got %zu", key, (size_t)(n), numel)
    if (m->rn && k.rfind("visual.", 0) == 0) rc = resnet_set_weight(m, k, data, numel);
    else if (k.rfind("visual.transformer.resblocks.", 0) == 0) rc = blk("visual.transformer.resblocks.", m->vis);
    else if (k.rfind("transformer.resblocks.", 0) == 0) rc = blk("transformer.resblocks.", m->txt);
    else if (k == "visual.conv1.weight") {
        EXPECT(dv * 3 * c.patch * c.patch);
        const size_t k0 = (size_t)3 * c.patch * c.patch, k0p = (size_t)patch_k0(c);
        std::vector<float> padded(dv * k0p, 0.f);  // rows zero-padded like the im2col rows
        for (size_t r = 0; r < dv; ++r) memcpy(&padded[r * k0p], data + r * k0, k0 * 4);
        rc = upload_lp(m->dtype, m->conv_w, nullptr, padded.data(), dv, k0p);
        if (!rc && m->conv_w8) rc = upload_e4m3(m->conv_w8, &m->conv_s8, padded.data(), dv, k0p);
    }
    else if (k == "visual.class_embedding") { EXPECT(dv); rc = upload_f32(m->cls, data, numel); }
    else if (k == "visual.positional_embedding") { EXPECT((1 + P) * dv); rc = upload_f32(m->vpos, data, numel); }
    else if (k == "visual.ln_pre.weight") { EXPECT(dv); rc = upload_f32(m->ln_pre_g, data, numel); }
    else if (k == "visual.ln_pre.bias") { EXPECT(dv); rc = upload_f32(m->ln_pre_b, data, numel); }
    else if (k == "visual.ln_post.weight") { EXPECT(dv); rc = upload_f32(m->ln_post_g, data, numel); }
    else if (k == "visual.ln_post.bias") { EXPECT(dv); rc = upload_f32(m->ln_post_b, data, numel); }
    else if (k == "visual.proj") { EXPECT(dv * e); rc = upload_f32(m->vproj, data, numel); }
    else if (k == "positional_embedding") { EXPECT((size_t)c.ctx_len * dt); rc = upload_f32(m->tpos, data, numel); if (!m->frozen) m->prompts_set = false; }  // frozen: added on the device at run time
    else if (k == "ln_final.weight") { EXPECT(dt); rc = upload_f32(m->ln_fin_g, data, numel); }
    else if (k == "ln_final.bias") { EXPECT(dt); rc = upload_f32(m->ln_fin_b, data, numel); }
    else if (k == "text_projection") { EXPECT(dt * e); rc = upload_f32(m->tproj, data, numel); }
    else if (k == "logit_scale") { EXPECT(1); m->scale = std::exp(data[0]); }  // trainers/mudpt.py:181
    else if (k == "token_embedding.weight" && m->frozen) {  // kept on the device: mudpt_set_text_tokens' prompts are embedded there
        ARG_CHECK(numel >= dt && numel % dt == 0 && numel / dt <= (size_t)0x7fffffff, "set_weight: %s expects [vocab, %zu], got %zu elements", key, dt, numel);
        if ((int)(numel / dt) != m->vocab) {  // the ids mudpt_set_text_tokens checked belong to the previous table
            if (m->tok_table) (void)hipFree(m->tok_table);
            m->tok_table = nullptr; m->vocab = 0; m->prompts_set = false;
            HIP_TRY(hipMalloc((void**)&m->tok_table, numel * 4));
            m->vocab = (int)(numel / dt);
        }
        rc = upload_f32(m->tok_table, data, numel);
    }
    else if (k == "token_embedding.weight" || k == "input_resolution" || k == "context_length" || k == "vocab_size") return MUDPT_OK;
    else { set_error("set_weight: unknown key '%s'", key); return MUDPT_ERR_ARG; }
#undef EXPECT
    if (rc) return rc;
    m->any_weight_set = true;
    if (m->vpt || m->frozen) m->text_valid = false;  // VPT / a frozen handle keep their text features across calls: any frozen weight may change them
    for (size_t i = 0; i < m->missing.size(); ++i)
        if (m->missing[i] == k) { m->missing.erase(m->missing.begin() + i); break; }
    return MUDPT_OK;
}

// CoOp's construct_prompts (trainers/coop.py:99-164), row by row: position of context row j, and the row of the TOKENIZED prompt
// "<X x n> <name>." that lands at prompt row t (context rows: t itself; their content is the spliced context).  suffix = rows 1 + n ..,
// h = n / 2 (rounded down, :122).  Rows from 1 + n + name_len on (".", EOT, padding) keep their place, so the EOT row does not move.
static int coop_ctx_row(int position, int n, int nl, int j) {
    if (position == MUDPT_CLASS_TOKEN_MIDDLE) return j < n / 2 ? 1 + j : 1 + nl + j;  // [SOS, ctx[:h], name, ctx[h:], suffix[nl:]]
    if (position == MUDPT_CLASS_TOKEN_FRONT) return 1 + nl + j;                          // [SOS, name, ctx, suffix[nl:]]
    return 1 + j;                                                                        // [SOS, ctx, suffix]
}
static int coop_src_row(int position, int n, int nl, int t) {
    const int h = n / 2;
    if (position == MUDPT_CLASS_TOKEN_MIDDLE && t >= 1 + h && t < 1 + h + nl) return 1 + n + (t - 1 - h);
    if (position == MUDPT_CLASS_TOKEN_FRONT && t >= 1 && t < 1 + nl) return 1 + n + (t - 1);
    return t;
}

extern "C" int mudpt_set_class_token_position(mudpt_model* m, int32_t position, const int32_t* name_lens) {
    ARG_CHECK(m, "set_class_token_position: null model");
    NOT_FROZEN(m, "set_class_token_position");
    ARG_CHECK(m->coop, "set_class_token_position: not a CoOp model (MUDPT_VARIANT_COOP / MUDPT_VARIANT_COOP_CSC)");
    ARG_CHECK(position == MUDPT_CLASS_TOKEN_END || position == MUDPT_CLASS_TOKEN_MIDDLE || position == MUDPT_CLASS_TOKEN_FRONT,
              "set_class_token_position: position %d is not MUDPT_CLASS_TOKEN_END / _MIDDLE / _FRONT", position);
    ARG_CHECK(name_lens || position == MUDPT_CLASS_TOKEN_END, "set_class_token_position: middle / front need name_lens");
    m->class_token_position = position;
    m->name_lens.clear();
    if (name_lens) m->name_lens.assign(name_lens, name_lens + m->cfg.n_cls);
    m->prompts_set = false;  // the row tables are built by the next mudpt_set_class_prompts
    m->text_valid = false;
    return MUDPT_OK;
}

// Length buckets (MuDPT, many classes): "a photo of a <name>." ends at position 7-9 for most ImageNet names and at 19 for a few; the
// caller's trim runs EVERY prompt to the longest.  Sorting the prompts by length and cutting the sorted list into <= txt_buckets groups,
// each run to its own longest member, removes most of the padding (C = 1000 synthetic names: 19 000 -> ~11 000 rows).  Sequences are
// independent in every kernel of the tower, so the kept rows are bit-identical to the single-bucket run (tests).  A bucket costs a
// handful of extra launches per block (attention, splice, reductions: ~1 000 rows' worth of time), which the cut search charges.
// The whole layout rule, pure host arithmetic (exported as mudpt_text_layout_plan), into *lay's host half.  eot [C]: the EOT position of every prompt;
// n_prompt: prompt rows per sequence; trim, max_buckets, bucket_cost: the knobs txt_trim, txt_buckets, txt_bucket_cost; allow_buckets: false for CoCoOp.
// The text tower is causal (clip/model.py:407-413) and only the EOT row of a prompt is used (trainers/mudpt.py:154): positions behind it influence no
// used output or gradient, so a sequence keeps max(eot + 1, n_prompt + 2) rows and a bucket runs to its longest member; trim = false: ctx_len rows, one bucket
struct TextPlan { std::vector<int> order, first, seg; };  // per packed sequence: its class, its first packed row, the index of its bucket
static TextPlan plan_text_layout(const int32_t* eot, int C, int ctx_len, int n_prompt, int heads, bool trim, int max_buckets, long bucket_cost, bool allow_buckets,
                                 TextLayout* lay) {
    TextPlan p;
    p.order.resize(C); p.first.resize(C); p.seg.resize(C);
    std::vector<int>& order = p.order;
    std::vector<TextLayout::Seg>& segs = lay->segs;
    segs.clear();
    for (int cc = 0; cc < C; ++cc) order[cc] = cc;
    auto len_of = [&](int cc) { return std::max(eot[cc] + 1, n_prompt + 2); };
    int Le = trim ? 0 : ctx_len;  // the kept length of the one-bucket run
    if (trim) for (int cc = 0; cc < C; ++cc) Le = std::max(Le, len_of(cc));
    if (allow_buckets && trim && max_buckets > 1 && (size_t)C * Le >= 2048) {
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return len_of(x) < len_of(y); });
        std::vector<int> dl, cnt;  // distinct lengths ascending, sequences per length
        for (int cc : order) {
            if (dl.empty() || dl.back() != len_of(cc)) { dl.push_back(len_of(cc)); cnt.push_back(0); }
            ++cnt.back();
        }
        const int nd = (int)dl.size(), K = std::min(max_buckets, nd);
        const long PEN = bucket_cost, INF = 1L << 60;
        std::vector<long> pre(nd + 1, 0);
        for (int j = 0; j < nd; ++j) pre[j + 1] = pre[j] + cnt[j];
        // best[b][j]: rows (+ penalties) of covering lengths 0..j-1 with b buckets, the last one ending at length j-1
        std::vector<std::vector<long>> best(K + 1, std::vector<long>(nd + 1, INF));
        std::vector<std::vector<int>> from(K + 1, std::vector<int>(nd + 1, 0));
        best[0][0] = 0;
        for (int bk = 1; bk <= K; ++bk)
            for (int j = 1; j <= nd; ++j)
                for (int i0 = bk - 1; i0 < j; ++i0) {
                    if (best[bk - 1][i0] >= INF) continue;
                    const long v = best[bk - 1][i0] + (pre[j] - pre[i0]) * dl[j - 1] + PEN;
                    if (v < best[bk][j]) { best[bk][j] = v; from[bk][j] = i0; }
                }
        int kb = 1;
        for (int bk = 2; bk <= K; ++bk) if (best[bk][nd] < best[kb][nd]) kb = bk;
        if (kb > 1) {
            std::vector<int> cuts;  // bucket boundaries in distinct-length indices
            for (int bk = kb, j = nd; bk >= 1; --bk) { cuts.push_back(j); j = from[bk][j]; }
            std::reverse(cuts.begin(), cuts.end());
            int j0 = 0, row0 = 0;
            size_t lse0 = 0;
            for (int j1 : cuts) {
                Tower::Seg g; g.row0 = row0; g.seq0 = (int)pre[j0]; g.nseq = (int)(pre[j1] - pre[j0]); g.L = dl[j1 - 1]; g.lse0 = lse0;
                segs.push_back(g);
                row0 += g.nseq * g.L;
                lse0 += (size_t)g.nseq * heads * attn_padded_len(g.L);
                j0 = j1;
            }
        } else {
            for (int cc = 0; cc < C; ++cc) order[cc] = cc;  // one bucket: keep the caller's order
        }
    }
    if (segs.empty()) { TextLayout::Seg one; one.nseq = C; one.L = Le; segs.push_back(one); }
    lay->L = Le; lay->nseq = C; lay->rows = segs.back().row0 + segs.back().nseq * segs.back().L;
    for (size_t b = 0; b < segs.size(); ++b)
        for (int j = 0; j < segs[b].nseq; ++j) { p.first[segs[b].seq0 + j] = segs[b].row0 + j * segs[b].L; p.seg[segs[b].seq0 + j] = (int)b; }
    return p;
}
// The device tables of a planned layout, sequence by sequence: perm, the EOT row of every sequence in the packed rows (rows) and relative to its
// bucket's first row (local); own(sequence, class, first row, rows of its bucket) adds the caller's.  lay.nseq > C: CoCoOp's chunk, see there
template <class F>
static void fill_layout_tables(const TextLayout& lay, const TextPlan& p, const int32_t* eot, int* perm, int* rows, int* local, F own) {
    const int C = (int)p.order.size(), per = lay.rows / (lay.nseq / C);  // packed rows of one image's class set
    for (int sq = 0; sq < lay.nseq; ++sq) {
        const TextLayout::Seg& g = lay.segs[p.seg[sq % C]];
        const int cc = p.order[sq % C], r0 = sq / C * per + p.first[sq % C];
        if (sq < C) perm[sq] = cc;
        rows[sq] = r0 + eot[cc]; local[sq] = rows[sq] - g.row0;
        own(sq, cc, (size_t)r0, g.L);
    }
}

// Points the text tower at a layout: what its block functions, tower_rows and TowerSegs read of it
static void bind_text_layout(Tower& t, const TextLayout& lay) { t.lay = &lay; t.L = lay.L; t.Lp = attn_padded_len(lay.L); t.tail_rows = lay.eot_rows; }

extern "C" int mudpt_set_class_prompts(mudpt_model* m, const float* emb, const int32_t* eot) {
    ARG_CHECK(m && emb && eot, "set_class_prompts: null argument");
    NOT_FROZEN(m, "set_class_prompts (a frozen handle takes token ids: mudpt_set_text_tokens)");
    m->cl_B = 0;  // the text tower's tables and activations may be rebuilt below: a mudpt_forward_train in flight ends here
    for (const std::string& k : m->missing)
        if (k == "positional_embedding") { set_error("set_class_prompts: set 'positional_embedding' first"); return MUDPT_ERR_STATE; }
    const mudpt_config& c = m->cfg;
    // emb / eot describe ALL n_cls classes on every rank; a class-sharded handle (mudpt_set_class_shard) keeps its own [c0, c0 + C) only
    const size_t C = (size_t)m->ct, c0 = (size_t)m->c0, L = c.ctx_len, d = c.t_width;
    for (int cc = 0; cc < c.n_cls; ++cc) ARG_CHECK(eot[cc] >= 0 && eot[cc] < (int)L, "set_class_prompts: eot index %d out of range", eot[cc]);
    emb += c0 * L * d;
    eot += c0;
    const int n = c.n_ctx, ctp = m->class_token_position;
    auto name_len = [&](size_t cc) { return m->name_lens.empty() ? 0 : m->name_lens[cc]; };
    if (m->coop) {  // every context row lies before the EOT row, which construct_prompts does not move
        for (size_t cc = 0; cc < C; ++cc)
            ARG_CHECK(name_len(cc) >= 0 && 1 + n + name_len(cc) <= eot[cc], "set_class_prompts: class %zu: name_lens %d with n_ctx %d does not fit before its EOT row %d",
                      cc, name_len(cc), n, eot[cc]);
    }
    Tower& X = m->txt; TextLayout& lay = m->lay;
    const TextPlan plan = plan_text_layout(eot, (int)C, c.ctx_len, X.n, X.heads, m->txt_trim, m->txt_buckets, m->txt_bucket_cost, !m->cocoop, &lay);
    const size_t Le = (size_t)lay.L, class_rows = (size_t)lay.rows;  // kept length; packed rows of the C class prompts
    // Sequences per text-tower pass.  MuDPT: the C class prompts.  CoCoOp: every image has its own C prompts (trainers/cocoop.py:187-194
    // loops over the images, C sequences at a time); here a CHUNK of images goes through the tower at once -- as many as fit a
    // memory budget (activations for the backward are ~150 KB per token at width 512) and the kernels' 32-bit offsets -- and
    // cocoop_forward / cocoop_forward_backward loop over the chunks.  The reference's own config (train batch 1, test batch 100, up to
    // 1000 classes) therefore needs C * Le tokens of activations at least, never max_batch * C * ctx_len.
    size_t chunk = 1;
    if (m->cocoop) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        for (void* p : m->txt.act_allocs) (void)hipFree(p);  // a previous sizing does not count against the budget
        m->txt.act_allocs.clear();
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t per_row = tower_bytes_per_row(m->txt), budget = (size_t)((double)free_b * 0.6);
        size_t rows_max = budget / per_row;
        // the widest row of a pass (QuickGELU(u) and its low half: 2 x 8 d bytes) stays inside the kernels' 32-bit byte offsets
        const size_t rows_cap = (size_t)0x7fffffff / ((size_t)16 * d) - 1;
        if (rows_max > rows_cap) rows_max = rows_cap;
        chunk = rows_max / (C * Le);
        if (chunk > (size_t)c.max_batch) chunk = (size_t)c.max_batch;
        if (m->cocoop_chunk > 0 && chunk > (size_t)m->cocoop_chunk) chunk = (size_t)m->cocoop_chunk;
        if (chunk < 1) {
            set_error("set_class_prompts: one image's %zu class prompts x %zu positions (%zu tokens, %.1f GB of text-tower activations) "
                      "exceed the budget of %.1f GB / %zu tokens per pass", C, Le, C * Le, (double)(C * Le * per_row) / 1e9, (double)budget / 1e9, rows_cap);
            return MUDPT_ERR_ARG;
        }
    }
    m->txt_chunk = (int)chunk;
    lay.segs[0].nseq *= (int)chunk; lay.nseq *= (int)chunk; lay.rows *= (int)chunk;  // CoCoOp: sequence i * C + c for image i of a chunk, one bucket
    if (int rc = alloc_tower_acts(m, X, lay.L, lay.nseq)) return rc;
    bind_text_layout(X, lay);
    std::vector<float> pos(L * d);
    HIP_TRY(hipMemcpy(pos.data(), m->tpos, pos.size() * 4, hipMemcpyDeviceToHost));
    std::vector<float> ep(class_rows * d);
    std::vector<int> rows(lay.nseq), rows_local(lay.nseq), tr((size_t)lay.nseq * X.n), perm(C), cpos(m->coop ? C * n : 0);
    int span = X.n;
    fill_layout_tables(lay, plan, eot, perm.data(), rows.data(), rows_local.data(), [&](int sq, int cc, size_t r0, int Lg) {
        if (!m->coop)
            for (int k = 0; k < X.n; ++k) tr[(size_t)sq * X.n + k] = (int)r0 + 1 + k;  // ctx rows 1..n (trainers/mudpt.py:97-115)
        if ((size_t)sq >= C) return;  // CoCoOp's further images: launch_cocoop_prompts builds their rows from these
        if (m->coop) {
            // CoOp: the prompt rows in construct_prompts' order, THEN the positional embedding (trainers/coop.py:187-188); the context
            // rows' table in the caller's class order, token rows of the packed layout (coop.hip)
            const int nl = name_len(cc);
            for (int k = 0; k < n; ++k) {
                cpos[(size_t)cc * n + k] = coop_ctx_row(ctp, n, nl, k);
                tr[(size_t)cc * n + k] = (int)r0 + cpos[(size_t)cc * n + k];
            }
            span = std::max(span, coop_ctx_row(ctp, n, nl, n - 1));
            for (int t = 0; t < Lg; ++t) {
                const float* src = emb + ((size_t)cc * L + coop_src_row(ctp, n, nl, t)) * d;
                for (size_t k = 0; k < d; ++k) ep[(r0 + t) * d + k] = src[k] + pos[(size_t)t * d + k];
            }
            return;
        }
        for (size_t i = 0; i < (size_t)Lg * d; ++i) ep[r0 * d + i] = emb[(size_t)cc * L * d + i] + pos[i];  // trainers/mudpt.py:143
    });
    HIP_TRY(hipMemcpy(m->emb_pos, ep.data(), ep.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lay.eot_rows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lay.eot_local, rows_local.data(), rows_local.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(m->tprompt_rows, tr.data(), tr.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(lay.perm, perm.data(), perm.size() * 4, hipMemcpyHostToDevice));
    if (m->coop) HIP_TRY(hipMemcpy(m->coop_pos, cpos.data(), cpos.size() * 4, hipMemcpyHostToDevice));
    X.head_span = span;  // block 0's backward computes the attention rows 1 .. span, which hold every context row (CoOp middle / front: > n)
    m->prompts_set = true;
    m->text_valid = false;
    return MUDPT_OK;
}

// Frozen handles: the class prompts of every template as token ids (trainers/zsclip.py:61-65,108-110).  Host work only until the tables are
// uploaded: the EOT position of a prompt (clip/model.py:836 text.argmax(dim=-1): the FIRST maximum), each template's layout by the rules of
// mudpt_set_class_prompts, and per packed token row its id and its position -- what embed_tokens_kernel turns into block 0's input.
extern "C" int mudpt_set_text_tokens(mudpt_model* m, const int32_t* tokens, int32_t n_templates) {
    ARG_CHECK(m && tokens, "set_text_tokens: null argument");
    ARG_CHECK(m->frozen, "set_text_tokens: not a frozen handle (mudpt_create_frozen); the other variants take mudpt_set_class_prompts");
    ARG_CHECK(n_templates >= 1, "set_text_tokens: n_templates %d must be >= 1", n_templates);
    bool pos_set = true;
    for (const std::string& k : m->missing) pos_set = pos_set && k != "positional_embedding";
    if (!m->tok_table || !pos_set) { set_error("set_text_tokens: set 'token_embedding.weight' and 'positional_embedding' first"); return MUDPT_ERR_STATE; }
    const mudpt_config& c = m->cfg;
    const size_t C = (size_t)c.n_cls, L = (size_t)c.ctx_len, T = (size_t)n_templates;
    for (size_t i = 0; i < T * C * L; ++i)
        ARG_CHECK(tokens[i] >= 0 && tokens[i] < m->vocab, "set_text_tokens: token id %d (template %zu, class %zu, position %zu) outside the %d rows of the embedding table",
                  tokens[i], i / (C * L), i / L % C, i % L, m->vocab);
    Tower& X = m->txt;
    std::vector<mudpt_model::Template> tm(T);
    std::vector<int> host;                          // every template's five tables, one behind the other
    std::vector<size_t> base(T);
    int Lmax = 0;
    for (size_t t = 0; t < T; ++t) {
        const int32_t* tk = tokens + t * C * L;
        std::vector<int32_t> eot(C);
        for (size_t cc = 0; cc < C; ++cc) {
            const int32_t* row = tk + cc * L;
            eot[cc] = (int32_t)(std::max_element(row, row + L) - row);  // the first of equal maxima
        }
        TextLayout& P = tm[t].lay;
        const TextPlan plan = plan_text_layout(eot.data(), (int)C, c.ctx_len, 0, X.heads, m->txt_trim, m->txt_buckets, m->txt_bucket_cost, true, &P);
        base[t] = host.size();
        host.resize(base[t] + 2 * (size_t)P.rows + 3 * C);
        int *tok = host.data() + base[t], *pos = tok + P.rows, *rows = pos + P.rows, *local = rows + C, *perm = local + C;
        fill_layout_tables(P, plan, eot.data(), perm, rows, local, [&](int, int cc, size_t r0, int Lg) {
            for (int l = 0; l < Lg; ++l) { tok[r0 + l] = tk[(size_t)cc * L + l]; pos[r0 + l] = l; }
        });
        Lmax = std::max(Lmax, P.L);
    }
    m->prompts_set = false;
    m->text_valid = false;
    // one set of activations for every template: n_cls sequences of the longest kept length hold any template's packed rows (the tower lets go of its layout here)
    if (int rc = alloc_tower_acts(m, X, Lmax, (int)C)) return rc;
    if (m->tmpl_tables) (void)hipFree(m->tmpl_tables);
    m->tmpl_tables = nullptr;
    m->tmpl.clear();
    HIP_TRY(hipMalloc((void**)&m->tmpl_tables, host.size() * 4));
    HIP_TRY(hipMemcpy(m->tmpl_tables, host.data(), host.size() * 4, hipMemcpyHostToDevice));
    for (size_t t = 0; t < T; ++t) {
        mudpt_model::Template& P = tm[t]; int* tables = m->tmpl_tables + base[t];
        P.tok = tables; P.pos = tables + P.lay.rows; P.lay.eot_rows = tables + 2 * P.lay.rows; P.lay.eot_local = P.lay.eot_rows + C; P.lay.perm = P.lay.eot_local + C;
    }
    m->tmpl = tm;
    m->prompts_set = true;
    return MUDPT_OK;
}

extern "C" int mudpt_text_layout(const mudpt_model* m, int32_t* rows, int32_t* buckets, int32_t* max_len) {
    ARG_CHECK(m && m->prompts_set, "text_layout: call mudpt_set_class_prompts (a frozen handle: mudpt_set_text_tokens) first");
    // over the handle's layouts (a frozen handle: one per template): token rows summed, the largest bucket count, the longest kept length
    int r = 0, b = 0, l = 0;
    auto add = [&](const TextLayout& t) { r += t.rows; b = std::max(b, (int)t.segs.size()); l = std::max(l, t.L); };
    if (!m->frozen) add(m->lay);
    for (const mudpt_model::Template& t : m->tmpl) add(t.lay);
    if (rows) *rows = r; if (buckets) *buckets = b; if (max_len) *max_len = l;
    return MUDPT_OK;
}

extern "C" int mudpt_param_count(const mudpt_model* m) { return m ? (int)m->tr.size() : 0; }
extern "C" size_t mudpt_param_numel(const mudpt_model* m) { return m ? m->total : 0; }
extern "C" int mudpt_param_info(const mudpt_model* m, int i, const char** name, size_t* offset, size_t* numel, int32_t* ndim, int64_t shape[3]) {
    ARG_CHECK(m && i >= 0 && i < (int)m->tr.size(), "param_info: bad index %d", i);
    const Trainable& t = m->tr[i];
    if (name) *name = t.name.c_str();
    if (offset) *offset = t.off;
    if (numel) *numel = t.numel;
    if (ndim) *ndim = t.ndim;
    if (shape) for (int k = 0; k < 3; ++k) shape[k] = t.shape[k];
    return MUDPT_OK;
}
extern "C" int mudpt_bind_params(mudpt_model* m, float* p, float* g) {
    NOT_FROZEN(m, "bind_params");
    ARG_CHECK(m && p, "bind_params: null argument");
    ARG_CHECK((uintptr_t)p % 16 == 0 && (uintptr_t)g % 16 == 0, "bind_params: buckets must be 16-byte aligned");
    m->cl_B = 0;  // the forward in flight ran on the old bucket's parameters
    m->params = p;
    m->grads = g;
    return MUDPT_OK;
}

// ---- the path ---------------------------------------------------------------------------------------------
#define TRY(expr)                      \
    do {                               \
        if (int _e = (expr)) return _e; \
    } while (0)

static int ready(mudpt_model* m, int B, bool need_grads) {
    ARG_CHECK(m, "null model");
    if (!m->missing.empty()) {
        set_error("model not ready: %zu frozen weights unset (first: %s)", m->missing.size(), m->missing[0].c_str());
        return MUDPT_ERR_STATE;
    }
    if (!m->prompts_set) { set_error("model not ready: call mudpt_set_class_prompts"); return MUDPT_ERR_STATE; }
    if (!m->params) { set_error("model not ready: call mudpt_bind_params"); return MUDPT_ERR_STATE; }
    if (need_grads && !m->grads) { set_error("model not ready: no gradient bucket bound"); return MUDPT_ERR_STATE; }
    ARG_CHECK(B > 0 && B <= m->cfg.max_batch, "batch %d outside 1..max_batch=%d", B, m->cfg.max_batch);
    return MUDPT_OK;
}

// Split operands: the form of the low half at GEMM site `site` of tower t whose contraction length is K (common.h LoMode) -- what the
// producing kernel writes and what the consuming GEMM's second pass reads.  The e4m3 pass needs K % 128 == 0 (one matrix instruction
// contracts 128 k): narrower sites of a LO_F8 tower (the 192-wide test shapes) fall back to the fp16 pair.
enum Site : int { SITE_QKV = 0, SITE_OUT = 1, SITE_FC = 2, SITE_PROJ = 3, SITE_PATCH = 4 };
static int site_mode(const Tower& t, int site, int K) {
    if (t.split == LO_NONE || !((t.sites >> site) & 1)) return LO_NONE;
    return (t.split == LO_F8 && K % 128 == 0) ? LO_F8 : LO_F16;
}
// ... and the second-pass fields of the consuming GEMM: the low half of A, and for the e4m3 form the e4m3 weights (same row offset as B) + scale
static void split_operand(GemmArgs& g, int mode, const void* A_lo, const void* B8, int b8_scale) {
    if (mode == LO_NONE) return;
    g.A_lo = A_lo; g.lo_mode = mode;
    if (mode == LO_F8) { g.B8 = B8; g.b8_scale = b8_scale; }
}

// ---- the steps of a block, each written once: block_fwd / block_fwd_tail / block_bwd_tail / block_bwd only sequence them ---------------
static const size_t kOpBytes = 2;  // one element of T
static char* lp_at(const void* p, size_t elems) { return (char*)p + elems * kOpBytes; }  // element `elems` of a T buffer
// compact rows of `width` elements of esz bytes: dst[r] = src[idx[r]] (gather), dst[idx[r]] = src[r] (scatter)
static int gather(const void* src, const int* idx, void* dst, int rows, int width, size_t esz, hipStream_t s) { return launch_gather_rows(src, width * esz, idx, dst, width * esz, rows, (int)(width * esz), s); }
static int scatter(const void* src, const int* idx, void* dst, int rows, int width, size_t esz, hipStream_t s) { return launch_scatter_rows(src, width * esz, idx, dst, width * esz, rows, (int)(width * esz), s); }
// ... into zeros: the other rows of dst [all_rows, width] get 0
static int scatter_zeroed(const void* src, const int* idx, void* dst, int all_rows, int rows, int width, size_t esz, hipStream_t s) {
    HIP_TRY(hipMemsetAsync(dst, 0, (size_t)all_rows * width * esz, s));
    return scatter(src, idx, dst, rows, width, esz, s);
}
// The buffers a half-step of a block works on, for a row set: every row of the pass (rows_all) or the last block's one used row per sequence,
// compact (rows_tail; Tower::tail_rows).  big: its LayerNorms go through ln_fwd_call / ln_bwd_call (bracketed when profiling); the tail's never do
struct BlockRows {
    int rows = 0; bool big = false;
    void *h = nullptr, *h_lo = nullptr, *g = nullptr, *g_lo = nullptr, *u = nullptr, *attn = nullptr, *attn_lo = nullptr;  // T
    float *x_in = nullptr, *x_mid = nullptr, *mean2 = nullptr, *rstd2 = nullptr, *dx = nullptr; void *dx_lp = nullptr, *dattn = nullptr;  // dx, dx_lp: the gradient stream (fp32 / T)
};
static BlockRows rows_all(const Tower& t, int i, int nseq) {
    const BlockAct& a = t.a[i];
    BlockRows r; r.rows = tower_rows(t, nseq); r.big = true; r.h = t.h; r.h_lo = t.h_lo; r.g = t.g; r.g_lo = t.g_lo; r.u = a.u; r.attn = a.attn; r.attn_lo = t.attn_lo;
    r.x_in = a.x_in; r.x_mid = a.x_mid; r.mean2 = a.mean2; r.rstd2 = a.rstd2; r.dx = t.dx; r.dx_lp = t.dx_lp; r.dattn = t.dattn;
    return r;
}
static BlockRows rows_tail(const Tower& t, int nseq) {
    const BlockAct& a = t.a[t.layers - 1];
    BlockRows r; r.rows = nseq; r.h = t.h_sel; r.h_lo = t.h_sel_lo; r.g = t.g_sel; r.g_lo = t.g_sel_lo; r.u = t.u_sel; r.attn = t.attn_sel; r.attn_lo = t.attn_sel_lo;
    r.x_in = t.xin_sel; r.x_mid = t.xmid_sel; r.mean2 = a.mean2; r.rstd2 = a.rstd2; r.dx = t.dsel; r.dx_lp = t.dsel_lp; r.dattn = t.dattn_sel;
    return r;
}
// Forward GEMM of a frozen Linear W [N, K] (+ bias) at split-operand site `site`; the caller adds the epilogue's operands (out0, aux)
static GemmArgs gemm_site(const Tower& t, int site, const void* A, const void* A_lo, int rows, const void* W, const void* W8, int s8, const float* bias, int N, int K) {
    GemmArgs g; g.A = A; g.lda = K; g.B = W; g.ldb = K; g.M = rows; g.N = N; g.K = K; g.bias = bias;
    split_operand(g, site_mode(t, site, K), A_lo, W8, s8); return g;
}
// in_proj, output features n0 .. n0 + N - 1 (q | k | v: rows of the weight, of its e4m3 copy and of the bias) of the ln_1 output h
static GemmArgs gemm_in_proj(const Tower& t, const BlockW& w, const void* h, const void* h_lo, int rows, int n0, int N) {
    const size_t o = (size_t)n0 * t.d;  // the same element offset into the e4m3 copy: its rows have the T copy's length in bytes
    return gemm_site(t, SITE_QKV, h, h_lo, rows, lp_at(w.w_in, o), w.w_in8 ? lp_at(w.w_in8, o) : nullptr, w.s_in8, w.b_in + n0, N, t.d);
}
static GemmArgs gemm_out_proj(const Tower& t, const BlockW& w, const BlockRows& r) { return gemm_site(t, SITE_OUT, r.attn, r.attn_lo, r.rows, w.w_out, w.w_out8, w.s_out8, w.b_out, t.d, t.d); }
static GemmArgs gemm_proj(const Tower& t, const BlockW& w, const BlockRows& r) { return gemm_site(t, SITE_PROJ, r.g, r.g_lo, r.rows, w.w_proj, w.w_proj8, w.s_proj8, w.b_proj, t.d, 4 * t.d); }
// c_fc + QuickGELU, complete: u (or, gelu_q8, byte codes of QuickGELU'(u): rows of 4 d bytes) for the backward, QuickGELU(u) (+ low half) for c_proj
static GemmArgs gemm_fc(const mudpt_model* m, const Tower& t, const BlockW& w, const BlockRows& r) {
    const int d = t.d, m_proj = site_mode(t, SITE_PROJ, 4 * d);
    GemmArgs f = gemm_site(t, SITE_FC, r.h, r.h_lo, r.rows, w.w_fc, w.w_fc8, w.s_fc8, w.b_fc, 4 * d, d);
    f.out0 = r.u; f.ldo0 = 4 * d; f.out1 = r.g; f.ldo1 = 4 * d; f.gelu_q8 = m->gelu_q8 && t.split == LO_NONE;
    if (m_proj != LO_NONE) { f.out1_lo = r.g_lo; f.out1_lo_mode = m_proj; }
    return f;
}
// dX [rows, N] = dY [rows, K] Wt^T against the transposed copy Wt [N, ldw] of a frozen Linear (K < ldw: a range of its output features)
static GemmArgs gemm_dx(const void* dY, int lddy, const void* Wt, int ldw, int rows, int N, int K, void* dX) {
    GemmArgs g; g.A = dY; g.lda = lddy; g.B = Wt; g.ldb = ldw; g.M = rows; g.N = N; g.K = K; g.out0 = dX; g.ldo0 = N; return g;
}
// ... in_proj's, from the K gradient columns k0 .. of q | k | v (dY points at the first of them)
static GemmArgs gemm_in_proj_dx(const Tower& t, const BlockW& w, const void* dY, int lddy, int rows, int k0, int K, void* dh) { return gemm_dx(dY, lddy, lp_at(w.w_in_t, k0), 3 * t.d, rows, t.d, K, dh); }
// ln_2 into the c_fc operand h (+ low half); the caller names the input: x alone (tail) or x + add -> xout (full rows)
static LnFwdArgs ln_2(const Tower& t, const BlockW& w, const BlockRows& r) {
    const int d = t.d, m_fc = site_mode(t, SITE_FC, d);
    LnFwdArgs l; l.ldx = d; l.gamma = w.ln2_g; l.beta = w.ln2_b; l.out = r.h; l.ldo = d; l.mean = r.mean2; l.rstd = r.rstd2; l.rows = r.rows; l.d = d;
    if (m_fc != LO_NONE) { l.out_lo = r.h_lo; l.lo_mode = m_fc; }
    return l;
}
// LayerNorm backward into the gradient stream, in place (in T alone when lp_grad; the T copy is always written).  The caller adds a row map
// (row_index / stats_by_token) or the splice's side output
static LnBwdArgs stream_ln_bwd(const mudpt_model* m, const Tower& t, const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* stream_f32, void* stream_lp, int rows) {
    const int d = t.d;
    LnBwdArgs b; b.dy = dy; b.lddy = d; b.x = x; b.ldx = d; b.mean = mean; b.rstd = rstd; b.gamma = gamma; b.lddres = d;
    if (m->lp_grad) b.dres_lp = stream_lp; else { b.dres = stream_f32; b.dx = stream_f32; }
    b.lddx = d; b.dx_lp = stream_lp; b.lddx_lp = d; b.rows = rows; b.d = d;
    return b;
}
// Attention operands of length bucket g.  saved: the block's attention output and log-sum-exp (the single-query forms keep theirs per sequence)
static AttnArgs seg_attn(const Tower& t, const BlockAct& a, const Tower::Seg& g, bool saved = true) {
    AttnArgs at; at.qkv = lp_at(a.qkv, (size_t)g.row0 * 3 * t.d); at.B = g.nseq; at.L = g.L; at.H = t.heads; at.causal = t.causal;
    if (saved) { at.out = lp_at(a.attn, (size_t)g.row0 * t.d); at.lse = a.lse + g.lse0; }
    return at;
}
static const int* seg_tail_rows(const Tower& t, const Tower::Seg& g) { return t.packed() ? t.lay->eot_local + g.seq0 : t.tail_rows; }  // packed: relative to the bucket

// Forward of the last block after its attention, on the one used row of every sequence (Tower::tail_rows): gathers the
// rows, then out_proj (+ residual in the small GEMM's epilogue), ln_2, c_fc + QuickGELU, c_proj (+ residual) -> t.xout_sel.
static int block_fwd_tail(mudpt_model* m, Tower& t, int nseq, hipStream_t s, bool attn_sel_ready = false) {
    const int i = t.layers - 1, d = t.d;
    const BlockW& w = t.w[i];
    const BlockRows r = rows_tail(t, nseq);
    if (!attn_sel_ready) {
        TRY(gather(t.a[i].attn, t.tail_rows, r.attn, nseq, d, kOpBytes, s));
        if (site_mode(t, SITE_OUT, d) != LO_NONE) TRY(gather(t.attn_lo, t.tail_rows, r.attn_lo, nseq, d, kOpBytes, s));
    }
    TRY(gather(t.a[i].x_in, t.tail_rows, r.x_in, nseq, d, 4, s));
    GemmArgs o = gemm_out_proj(t, w, r); o.out0 = r.x_mid; o.ldo0 = d; o.aux = r.x_in; o.ldaux = d;
    TRY(gemm_call(m, EPI_RESIDUAL, o, s));
    LnFwdArgs l2 = ln_2(t, w, r); l2.x = r.x_mid;
    TRY(launch_ln_fwd(m->dtype, l2, s));
    TRY(gemm_call(m, EPI_GELU, gemm_fc(m, t, w, r), s));
    GemmArgs p = gemm_proj(t, w, r); p.out0 = t.xout_sel; p.ldo0 = d; p.aux = r.x_mid; p.ldaux = d;
    return gemm_call(m, EPI_RESIDUAL, p, s);
}

// Block i of a tower.  The residual adds are NOT in the GEMM epilogues: out_proj / c_proj write their fp32 result
// (+ bias) to t.upd and the FOLLOWING LayerNorm kernel adds it to the stream while it reads it (the stream has to
// pass through that kernel anyway; a GEMM epilogue that loads the residual stalls behind its own stores, since
// vmcnt retires in order).  So LN1 of block i >= 1 computes x_in[i] = x_mid[i-1] + upd, with the deep-prompt rows
// spliced in (splice != null), and writes it for the backward; LN2 computes x_mid[i] = x_in[i] + upd.
static int block_fwd(mudpt_model* m, Tower& t, int i, int nseq, const float* splice, hipStream_t s) {
    const BlockRows r = rows_all(t, i, nseq);
    const int M = r.rows, d = t.d, dt = m->dtype, n = t.n;
    const TowerSegs segs(t, nseq);
    // bf16 mode: the update stream (out_proj / c_proj results) is kept in T like the gradient stream -- half the store time
    // of those GEMMs and 2 bytes less per element in the LayerNorm that adds it.  The last block's c_proj stays fp32 (launch_add).
    const bool lp = m->lp_upd;
    const BlockW& w = t.w[i]; const BlockAct& a = t.a[i];
    // split operands (Tower::split): the form of the low half the producers of in_proj's / out_proj's operand write (LO_NONE: the site runs on T alone)
    const int m_qkv = site_mode(t, SITE_QKV, d), m_out = site_mode(t, SITE_OUT, d);
    LnFwdArgs l1; l1.x = a.x_in; l1.ldx = d; l1.gamma = w.ln1_g; l1.beta = w.ln1_b; l1.out = t.h; l1.ldo = d; l1.mean = a.mean1; l1.rstd = a.rstd1; l1.rows = M; l1.d = d;
    if (m_qkv != LO_NONE) { l1.out_lo = t.h_lo; l1.lo_mode = m_qkv; }
    if (i > 0) {
        l1.x = t.a[i - 1].x_mid; l1.ldadd = d; l1.xout = a.x_in; l1.ldxout = d;
        if (lp) l1.add_lp = t.upd; else l1.add = t.upd;
        if (splice) { l1.ov_rows = splice; l1.ov_row0 = t.prompt_row0; l1.ov_n = n; l1.ov_L = t.L; }
    }
    if (splice && i > 0 && t.packed()) {
        // the splice replaces rows by their position inside a sequence: one launch per length bucket
        for (const Tower::Seg& g : segs) {
            LnFwdArgs b = l1;
            const size_t r0 = (size_t)g.row0;
            b.x = l1.x + r0 * l1.ldx; b.xout = l1.xout + r0 * l1.ldxout;
            if (l1.add) b.add = l1.add + r0 * l1.ldadd;
            if (l1.add_lp) b.add_lp = lp_at(l1.add_lp, r0 * l1.ldadd);
            b.out = lp_at(l1.out, r0 * l1.ldo);
            if (l1.out_lo) b.out_lo = lp_at(l1.out_lo, r0 * l1.ldo);
            b.mean = l1.mean + r0; b.rstd = l1.rstd + r0; b.rows = g.nseq * g.L; b.ov_L = g.L;
            TRY(ln_fwd_call(m, t, b, s));
        }
    } else {
        TRY(ln_fwd_call(m, t, l1, s));
    }
    if (i + 1 == t.layers && m->last_single && !t.exact_attn && t.tail_rows) {
        // Last block: only ONE query per sequence is ever used (CLS / EOT row).  K and V for every row (the k, v thirds of in_proj: rows
        // d .. 3d of its weight, written into the k, v thirds of the packed qkv buffer), q for the selected rows only, single-query attention
        // straight into the compact attn_sel the tail works on.  (With the fp32 attention forward the general kernel runs instead: the
        // single-query kernels take fp16 q, k, v.)
        GemmArgs kv = gemm_in_proj(t, w, t.h, t.h_lo, M, d, 2 * d); kv.out0 = lp_at(a.qkv, d); kv.ldo0 = 3 * d;
        TRY(gemm_call(m, EPI_STORE, kv, s));
        TRY(gather(t.h, t.tail_rows, t.h_sel, nseq, d, kOpBytes, s));
        if (m_qkv != LO_NONE) TRY(gather(t.h_lo, t.tail_rows, t.h_sel_lo, nseq, d, kOpBytes, s));
        GemmArgs qs = gemm_in_proj(t, w, t.h_sel, t.h_sel_lo, nseq, 0, d); qs.out0 = t.q_sel; qs.ldo0 = d;
        TRY(gemm_call(m, EPI_STORE, qs, s));
        for (const Tower::Seg& g : segs) {
            const size_t q0 = (size_t)g.seq0 * d;
            AttnArgs at = seg_attn(t, a, g, false); at.sel_rows = seg_tail_rows(t, g); at.lo_mode = m_out;
            TRY(launch_attn_fwd_single(dt, at, lp_at(t.q_sel, q0), lp_at(t.attn_sel, q0), m_out != LO_NONE ? lp_at(t.attn_sel_lo, q0) : nullptr, d,
                                       t.lse_sel + (size_t)g.seq0 * t.heads, s));
        }
        return block_fwd_tail(m, t, nseq, s, true);
    }
    GemmArgs q = gemm_in_proj(t, w, t.h, t.h_lo, M, 0, 3 * d); q.out0 = a.qkv; q.ldo0 = 3 * d;
    if (t.exact_attn) q.out0 = t.qkv32;  // fp32 q | k | v for the fp32 attention forward, which leaves their fp16 copy in a.qkv for the backward
    TRY(gemm_call(m, t.exact_attn ? EPI_STORE_F32 : EPI_STORE, q, s));
    for (const Tower::Seg& g : segs) {
        AttnArgs at = seg_attn(t, a, g);
        if (m_out != LO_NONE) { at.out_lo = lp_at(t.attn_lo, (size_t)g.row0 * d); at.lo_mode = m_out; }
        if (t.exact_attn) { at.qkv32 = t.qkv32 + (size_t)g.row0 * 3 * d; at.qkv_lp = lp_at(a.qkv, (size_t)g.row0 * 3 * d); }
        TRY(attn_call(m, t, at, false, s));
    }
    if (i + 1 == t.layers) return block_fwd_tail(m, t, nseq, s);
    const bool fs = !t.causal && t.split == LO_NONE;  // forward split K: the vision tower's out_proj / c_proj at tiny batches only (gemm_call), never with split operands
    GemmArgs o = gemm_out_proj(t, w, r); o.out0 = t.upd; o.ldo0 = d;
    TRY(gemm_call(m, lp ? EPI_STORE : EPI_STORE_F32, o, s, false, fs));
    LnFwdArgs l2 = ln_2(t, w, r); l2.x = r.x_in; if (lp) l2.add_lp = t.upd; else l2.add = t.upd; l2.ldadd = d; l2.xout = r.x_mid; l2.ldxout = d;
    TRY(ln_fwd_call(m, t, l2, s));
    TRY(gemm_call(m, EPI_GELU, gemm_fc(m, t, w, r), s));
    GemmArgs p = gemm_proj(t, w, r); p.out0 = t.upd; p.ldo0 = d;
    return gemm_call(m, lp ? EPI_STORE : EPI_STORE_F32, p, s, false, fs);
}

// Backward of a block from its output to its attention output, on a row set: c_proj dX with QuickGELU' (as the forward stored it, gemm_fc),
// c_fc dX, ln_2 backward into the gradient stream r.dx / r.dx_lp (then the gradient w.r.t. x_mid), out_proj dX -> r.dattn
static int mlp_bwd(mudpt_model* m, Tower& t, int i, const BlockRows& r, hipStream_t s) {
    const int d = t.d; const BlockW& w = t.w[i];
    GemmArgs g1 = gemm_dx(r.dx_lp, d, w.w_proj_t, d, r.rows, 4 * d, d, r.g); g1.aux = r.u; g1.ldaux = 4 * d; g1.gelu_q8 = m->gelu_q8 && t.split == LO_NONE;
    TRY(gemm_call(m, EPI_GELU_BWD, g1, s, !t.causal));
    TRY(gemm_call(m, EPI_STORE, gemm_dx(r.g, 4 * d, w.w_fc_t, 4 * d, r.rows, d, 4 * d, r.h), s, !t.causal));
    const LnBwdArgs b2 = stream_ln_bwd(m, t, r.h, r.x_mid, r.mean2, r.rstd2, w.ln2_g, r.dx, r.dx_lp, r.rows);
    TRY(r.big ? ln_bwd_call(m, t, b2, s) : launch_ln_bwd(m->dtype, b2, s));
    return gemm_call(m, EPI_STORE, gemm_dx(r.dx_lp, d, w.w_out_t, d, r.rows, d, d, r.dattn), s, !t.causal);
}

// Backward of the last block's tail (see Tower::tail_rows).  in: t.dsel / t.dsel_lp = gradient w.r.t. the selected rows of
// the tower output; out: t.dx / t.dx_lp = gradient w.r.t. the last block's input, all rows.
static int block_bwd_tail(mudpt_model* m, Tower& t, int nseq, hipStream_t s) {
    const int i = t.layers - 1, M = tower_rows(t, nseq), S = nseq, d = t.d, dt = m->dtype;
    const TowerSegs segs(t, nseq);
    const BlockW& w = t.w[i]; const BlockAct& a = t.a[i];
    TRY(mlp_bwd(m, t, i, rows_tail(t, nseq), s));  // t.dsel(_lp) = gradient w.r.t. x_mid on the selected rows
    if (m->last_single && !t.exact_attn) {
        // single-query attention backward: dK, dV of every row (k, v thirds of t.dqkv) and dq of the one query per sequence
        for (const Tower::Seg& g : segs) {
            const size_t q0 = (size_t)g.seq0 * d;
            AttnArgs at = seg_attn(t, a, g, false); at.dqkv = lp_at(t.dqkv, (size_t)g.row0 * 3 * d); at.sel_rows = seg_tail_rows(t, g);
            TRY(launch_attn_bwd_single(dt, at, lp_at(t.q_sel, q0), lp_at(t.attn_sel, q0), d, lp_at(t.dattn_sel, q0), t.lse_sel + (size_t)g.seq0 * t.heads,
                                       lp_at(t.dq_sel, q0), s));
        }
        // d(ln_1 output) = dK, dV rows . W_kv  (K range d .. 3d of the transposed in_proj weight)  +  on the selected rows  dq . W_q
        TRY(gemm_call(m, EPI_STORE, gemm_in_proj_dx(t, w, lp_at(t.dqkv, d), 3 * d, M, d, 2 * d, t.h), s, !t.causal));
        TRY(gemm_call(m, EPI_STORE, gemm_in_proj_dx(t, w, t.dq_sel, d, S, 0, d, t.dqx_sel), s, !t.causal));
        TRY(launch_add_rows(dt, t.dqx_sel, t.tail_rows, t.h, S, d, s));
    } else {
        // attention backward over all keys: d(attention output) is zero except on the selected query rows
        TRY(scatter_zeroed(t.dattn_sel, t.tail_rows, t.dattn, M, S, d, kOpBytes, s));
        for (const Tower::Seg& g : segs) {
            AttnArgs at = seg_attn(t, a, g);
            at.dout = lp_at(t.dattn, (size_t)g.row0 * d); at.dqkv = lp_at(t.dqkv, (size_t)g.row0 * 3 * d); at.delta = t.delta + g.lse0;
            at.sel_rows = seg_tail_rows(t, g);  // d(attention output) is zero except on those rows: the kernels skip the all-zero query blocks
            TRY(attn_call(m, t, at, true, s));
        }
        TRY(gemm_call(m, EPI_STORE, gemm_in_proj_dx(t, w, t.dqkv, 3 * d, M, 0, 3 * d, t.h), s, !t.causal));
    }
    // the residual path into ln_1's input: d(x_mid), zero except on the selected rows
    TRY(scatter_zeroed(t.dsel_lp, t.tail_rows, t.dx_lp, M, S, d, kOpBytes, s));
    if (!m->lp_grad) TRY(scatter_zeroed(t.dsel, t.tail_rows, t.dx, M, S, d, 4, s));
    return ln_bwd_call(m, t, stream_ln_bwd(m, t, t.h, a.x_in, a.mean1, a.rstd1, w.ln1_g, t.dx, t.dx_lp, M), s);
}

// Backward of block i (the last one: block_bwd_tail).  in: t.dx / t.dx_lp = gradient w.r.t. the block output; out: the same buffers = gradient w.r.t. x_in
// side != null: block i's input had deep-prompt rows spliced in; their gradient goes to side[seq][n_ctx][d] (row stride side_ldb per sequence) and the
// stream gets zeros on those rows (LnBwdArgs::side).  The last block's ln_1 backward is not fused with the splice: it ignores side and leaves them in the stream
static int block_bwd(mudpt_model* m, Tower& t, int i, int nseq, hipStream_t s, float* side = nullptr, size_t side_ldb = 0) {
    if (i == t.layers - 1) return block_bwd_tail(m, t, nseq, s);
    const int M = tower_rows(t, nseq), d = t.d;
    const BlockW& w = t.w[i]; const BlockAct& a = t.a[i];
    TRY(mlp_bwd(m, t, i, rows_all(t, i, nseq), s));
    const TowerSegs segs(t, nseq);
    for (const Tower::Seg& g : segs) {
        AttnArgs at = seg_attn(t, a, g);
        at.dout = lp_at(t.dattn, (size_t)g.row0 * d); at.dqkv = lp_at(t.dqkv, (size_t)g.row0 * 3 * d); at.delta = t.delta + g.lse0;
        // block 0: only the prompt rows of dqkv are read below (Tower::head_rows)
        if (i == 0 && t.head_rows && t.layers > 1 && m->attn_window) {
            at.win_row0 = t.prompt_row0;
            at.win_n = std::min(t.head_span > 0 ? t.head_span : t.head_n, g.L - t.prompt_row0);  // a bucket's head rows lie before its EOT rows
        }
        TRY(attn_call(m, t, at, true, s));
    }
    if (i == 0 && t.head_rows && t.layers > 1) {
        // block 0: d(x_in) on the prompt rows only (Tower::head_rows); the other rows of t.dx / t.dx_lp are left stale and
        // nothing reads them (the splice reductions and ln_pre's backward touch prompt rows only)
        const int R = nseq * t.head_n;
        TRY(gather(t.dqkv, t.head_rows, t.hd_dqkv, R, 3 * d, kOpBytes, s));
        TRY(gemm_call(m, EPI_STORE, gemm_in_proj_dx(t, w, t.hd_dqkv, 3 * d, R, 0, 3 * d, t.hd_h), s, !t.causal));
        LnBwdArgs b1 = stream_ln_bwd(m, t, t.hd_h, a.x_in, a.mean1, a.rstd1, w.ln1_g, t.dx, t.dx_lp, R); b1.row_index = t.head_rows; b1.stats_by_token = true;
        return launch_ln_bwd(m->dtype, b1, s);
    }
    TRY(gemm_call(m, EPI_STORE, gemm_in_proj_dx(t, w, t.dqkv, 3 * d, M, 0, 3 * d, t.h), s, !t.causal));
    LnBwdArgs b1 = stream_ln_bwd(m, t, t.h, a.x_in, a.mean1, a.rstd1, w.ln1_g, t.dx, t.dx_lp, M);
    if (side) { b1.side = side; b1.side_row0 = t.prompt_row0; b1.side_n = t.n; b1.side_L = t.L; b1.side_ldb = side_ldb; }
    return ln_bwd_call(m, t, b1, s);
}

// Where a tower's prompt rows come from and where their gradients are reduced to, resolved per call (mudpt_bind_params may rebind the
// buckets).  The one place that knows which variant keeps them where; a tower without prompt rows has no route.
struct PromptRoute {
    const float* in0 = nullptr;      // the n rows spliced at the tower's input
    const float* in0_add = nullptr;  // what is added to them
    const float* deep = nullptr;     // the [D1][n][d] rows of blocks 1 .. D1
    float* d_in0 = nullptr;          // where the gradient of in0 is reduced to
    float* d_deep = nullptr;         // where the gradient of deep is reduced to
};
static PromptRoute prompt_route(const mudpt_model* m, const Tower& t) {
    PromptRoute r;
    if (t.n == 0) return r;
    const bool vision = &t == &m->vis;
    const size_t group = (size_t)t.n * t.d;  // one block's rows
    float* P = m->params;
    auto G = [&](size_t o) { return m->grads ? m->grads + o : nullptr; };  // inference binds no gradient bucket
    if (!vision) r.in0_add = m->tpos + t.d;  // rows 1..n with the positional embedding (trainers/mudpt.py:97-115,143, mpt.py:108-125)
    if (m->indep) {
        // VPT / MPT: the tower's visual_ctx and, right behind it, its blocks' own visual_ctx, read from and reduced into the buckets directly
        // (clip/model.py:463-465)
        const size_t o = m->off(vision ? m->tr_vis0 : m->tr_txt0);
        r.in0 = P + o; r.deep = P + o + group; r.d_in0 = G(o); r.d_deep = G(o + group);
    } else if (m->umudpt && vision) {
        // the generator's output G [depth][n][dv]: row group 0 the input rows (alone: the tower has no visual_ctx of its own, clip/model.py:573-576),
        // 1 .. the deep prompts (:556-597); pg_dG collects the gradients likewise and the generator's backward reads it
        r.in0 = m->pg_G; r.deep = m->pg_G + group; r.d_in0 = m->pg_dG; r.d_deep = m->pg_dG + group;
        // UUMuDPT: G[0] + visual_ctx and G[1:] + visual_ctx_deep_prompts (clip/model.py:637-640; the sum uumudpt_forward_vision left in vis_deep).
        // Both are plain sums, so pg_dG is also the tower's term of grad(visual_ctx | visual_ctx_deep_prompts) (uumudpt_backward)
        if (m->uumudpt) { r.in0_add = P + m->off(UU_VCTX); r.deep = m->vis_deep; }
    } else if (vision) {  // MuDPT: visual_ctx + shared (clip/model.py:534) and the prompt learner's projections; gradients into its backward
        r.in0 = P + m->off(P_VCTX); r.in0_add = m->shared; r.deep = m->vis_deep; r.d_in0 = m->d_vprompt0; r.d_deep = m->d_vis_deep;
    } else {  // MuDPT / UMuDPT: ctx, its gradient summed over the class prompts straight into the bucket
        r.in0 = P + m->off(P_CTX); r.d_in0 = G(m->off(P_CTX));
        // UMuDPT: deep_prompts as they are in the bucket (trainers/umudpt.py:178,222); MuDPT: the prompt learner's sums; UUMuDPT: deep_prompts +
        // Gen2's output (uumudpt_forward_text), d_txt_deep then is dT as well as the text tower's term of grad(deep_prompts)
        const bool bucket = m->umudpt && !m->uumudpt;
        r.deep = bucket ? P + m->off(P_DEEP) : m->txt_deep;
        r.d_deep = bucket ? G(m->off(P_DEEP)) : m->d_txt_deep;
    }
    return r;
}

// The head of a tower: final LayerNorm on the used rows (t.xout_sel) and the projection proj [d, e] to the embedding (fp32; clip/model.py:549-552, trainers/mudpt.py:154-156).
// y / dy and the statistics hold one row per sequence of a step; a pass works on `rows` of them from row r0 on (CoCoOp's chunks); feat / dfeat [rows, e] are the caller's
struct TowerHead { const float *ln_g, *ln_b, *proj; float *mean, *rstd, *y, *dy; };
static TowerHead vision_head(const mudpt_model* m) { return {m->ln_post_g, m->ln_post_b, m->vproj, m->post_mean, m->post_rstd, m->f_ln, m->df_ln}; }
static TowerHead text_head(const mudpt_model* m) { return {m->ln_fin_g, m->ln_fin_b, m->tproj, m->fin_mean, m->fin_rstd, m->t_ln, m->dt_ln}; }
static int tower_head_fwd(mudpt_model* m, const Tower& t, const TowerHead& h, float* feat, int rows, size_t r0, hipStream_t s) {
    const int d = t.d, e = m->cfg.embed_dim;
    LnFwdArgs l; l.x = t.xout_sel; l.ldx = d; l.gamma = h.ln_g; l.beta = h.ln_b; l.out = h.y + r0 * d; l.ldo = d; l.out_f32 = true; l.mean = h.mean + r0; l.rstd = h.rstd + r0; l.rows = rows; l.d = d;
    TRY(launch_ln_fwd(m->dtype, l, s));
    return launch_sgemm(false, false, rows, e, d, 1.f, h.y + r0 * d, d, h.proj, e, 0.f, feat, e, nullptr, s);
}
// ... and its backward: dfeat -> t.dsel / t.dsel_lp, the gradient stream on the last block's tail rows
static int tower_head_bwd(mudpt_model* m, const Tower& t, const TowerHead& h, const float* dfeat, int rows, size_t r0, hipStream_t s) {
    const int d = t.d, e = m->cfg.embed_dim;
    TRY(launch_sgemm(false, true, rows, d, e, 1.f, dfeat, e, h.proj, e, 0.f, h.dy + r0 * d, d, nullptr, s));
    LnBwdArgs b; b.dy = h.dy + r0 * d; b.lddy = d; b.dy_f32 = true; b.x = t.xout_sel; b.ldx = d; b.mean = h.mean + r0; b.rstd = h.rstd + r0;
    b.gamma = h.ln_g; b.dx = m->lp_grad ? nullptr : t.dsel; b.lddx = d; b.dx_lp = t.dsel_lp; b.lddx_lp = d; b.rows = rows; b.d = d;
    return launch_ln_bwd(m->dtype, b, s);
}

// The gradient stream as the reductions behind a tower's backward read it, from token row row0 on: the fp32 copy, or (lp_grad) the T copy alone
struct GradStream { float* f32; void* lp; };
static GradStream grad_stream(const mudpt_model* m, const Tower& t, size_t row0 = 0) { return m->lp_grad ? GradStream{nullptr, lp_at(t.dx_lp, row0 * t.d)} : GradStream{t.dx + row0 * t.d, nullptr}; }
// Deep-prompt rows a tower consumed of D1 layers' worth: blocks >= depth never splice one, so rows used .. R of a [R, d] prompt-gradient table stay zero
static int used_prompt_rows(const Tower& t, int D1) { return (t.layers - 1 < D1 ? t.layers - 1 : D1) * t.n; }
static int zero_unused_rows(float* dprompt, int used, int R, int d, hipStream_t s) {
    if (used < R) HIP_TRY(hipMemsetAsync(dprompt + (size_t)used * d, 0, (size_t)(R - used) * d * 4, s));
    return MUDPT_OK;
}

// ---- the ResNet image tower (clip/model.py:17-161), NHWC in T; the rounding sites: resnet.hip's header ----
// One folded convolution: `in` is B images of H x H pixels with cin channels at channel stride ld_in (or, planar, the fp32 pixels); a 3 x 3 takes
// its patch rows, a 1 x 1 the activation as it lies (its K = ldk may reach past cin into the producer's zero channels).  out [B Ho Ho, np] =
// T(act(acc + bias + residual))
static int resnet_conv(mudpt_model* m, const RnConv& c, const void* in, int ld_in, bool planar, int B, int H, int stride, const void* res, int ldres, bool relu,
                       void* out, hipStream_t s) {
    Resnet& r = *m->rn;
    const int Ho = c.k == 3 ? (H - 1) / stride + 1 : H, M = B * Ho * Ho;
    if (r.conv_path == 1) {
        ++r.conv2d_launches;
        // the planar pixels (3 channels) keep their patch rows; the kernel then runs over them as a 1 x 1 whose channels are the ldk columns
        if (planar) {
            TRY(launch_im2col(m->dtype, in, true, B, H, H, c.cin, ld_in, stride, r.rows, c.ldk, s));
            return launch_conv2d(m->dtype, r.rows, B, Ho, Ho, c.ldk, c.ldk, 1, 1, c.w_dev, c.ldk, c.b_dev, res, ldres, out, c.np, c.np, relu, s);
        }
        return launch_conv2d(m->dtype, in, B, H, H, c.cin, ld_in, c.k, c.k == 3 ? stride : 1, c.w_dev, c.ldk, c.b_dev, res, ldres, out, c.np, c.np, relu, s);
    }
    GemmArgs g;
    if (c.k == 3) {
        TRY(launch_im2col(m->dtype, in, planar, B, H, H, c.cin, ld_in, stride, r.rows, c.ldk, s));
        g.A = r.rows; g.lda = c.ldk;
    } else {
        ARG_CHECK(ld_in >= c.ldk, "resnet: %s reads %d channels of an activation with %d", c.conv.c_str(), c.ldk, ld_in);
        g.A = in; g.lda = ld_in;
    }
    g.B = c.w_dev; g.ldb = c.ldk; g.M = M; g.N = c.np; g.K = c.ldk; g.out0 = r.acc; g.ldo0 = c.np;
    TRY(gemm_call(m, EPI_STORE_F32, g, s));
    return launch_bias_act(m->dtype, r.acc, c.np, c.b_dev, res, ldres, out, c.np, M, c.np, relu, s);
}

// ModifiedResNet.forward (clip/model.py:145-161) in eval mode -> m->img_f [B, e]
static int resnet_forward(mudpt_model* m, const float* images, int B, hipStream_t s) {
    Resnet& r = *m->rn;
    if (r.stale) TRY(resnet_fold(m, s));
    const int dt = m->dtype, e = m->cfg.embed_dim, C = r.C, L = r.L;
    void *X = r.act[0], *Y = r.act[1], *T1 = r.act[2], *T2 = r.act[3], *T3 = r.act[4], *ID = r.act[5], *XP = r.act[6];
    // the stem (:146-151): three 3 x 3 convolutions, the first of stride 2 on the pixels, and AvgPool2d(2)
    int H = r.S / 2;
    TRY(resnet_conv(m, r.convs[0], images, 0, true, B, r.S, 2, nullptr, 0, true, T1, s));
    TRY(resnet_conv(m, r.convs[1], T1, r.convs[0].np, false, B, H, 1, nullptr, 0, true, T2, s));
    TRY(resnet_conv(m, r.convs[2], T2, r.convs[1].np, false, B, H, 1, nullptr, 0, true, T1, s));
    int ldx = r.convs[2].np;
    TRY(launch_avgpool2d(dt, T1, ldx, X, ldx, B, H, H, ldx, 2, s));
    H /= 2;
    // the four stages of Bottleneck (:49-62)
    for (const RnBlock& b : r.blocks) {
        const RnConv &c1 = r.convs[b.conv1], &c2 = r.convs[b.conv2], &c3 = r.convs[b.conv3];
        const int Ho = H / b.stride;
        TRY(resnet_conv(m, c1, X, ldx, false, B, H, 1, nullptr, 0, true, T1, s));
        TRY(resnet_conv(m, c2, T1, c1.np, false, B, H, 1, nullptr, 0, true, T2, s));
        const void* t = T2;
        if (b.stride > 1) { TRY(launch_avgpool2d(dt, T2, c2.np, T3, c2.np, B, H, H, c2.np, b.stride, s)); t = T3; }
        const void* id = X;
        int ldid = ldx;
        if (b.down >= 0) {
            const RnConv& cd = r.convs[b.down];
            const void* x = X;
            if (b.stride > 1) { TRY(launch_avgpool2d(dt, X, ldx, XP, ldx, B, H, H, ldx, b.stride, s)); x = XP; }
            TRY(resnet_conv(m, cd, x, ldx, false, B, Ho, 1, nullptr, 0, false, ID, s));
            id = ID; ldid = cd.np;
        }
        TRY(resnet_conv(m, c3, t, c2.np, false, B, Ho, 1, id, ldid, true, Y, s));
        std::swap(X, Y);
        ldx = c3.np; H = Ho;
    }
    // AttentionPool2d (:75-98): the mean token in front, + positional_embedding; q from the mean token alone, k / v from all L tokens
    ARG_CHECK(ldx == C && H * H + 1 == L, "resnet: the tower ends at %d x %d x %d, the attention pool expects %d tokens of %d", H, H, ldx, L, C);
    TRY(launch_attnpool_tokens(dt, X, ldx, r.pos, r.tok, C, B, L - 1, C, s));
    GemmArgs q; q.A = r.tok; q.lda = L * C; q.B = r.w_q; q.ldb = C; q.M = B; q.N = C; q.K = C; q.bias = r.b_q; q.out0 = r.q; q.ldo0 = C;
    TRY(gemm_call(m, EPI_STORE_F32, q, s));
    GemmArgs kv; kv.A = r.tok; kv.lda = C; kv.B = r.w_kv; kv.ldb = C; kv.M = B * L; kv.N = 2 * C; kv.K = C; kv.bias = r.b_kv; kv.out0 = r.kv; kv.ldo0 = 2 * C;
    TRY(gemm_call(m, EPI_STORE_F32, kv, s));
    TRY(launch_attnpool_attend(dt, r.q, C, r.kv, r.kv + C, 2 * C, r.ao, C, B, L, r.shape.heads, s));
    GemmArgs cp; cp.A = r.ao; cp.lda = C; cp.B = r.w_c; cp.ldb = C; cp.M = B; cp.N = e; cp.K = C; cp.bias = r.b_c; cp.out0 = m->img_f; cp.ldo0 = e;
    return gemm_call(m, EPI_STORE_F32, cp, s);
}

// Vision tower forward, clip/model.py:526-553 (MuDPT: prompt rows appended before ln_pre, deep prompts spliced per block) or
// clip/model.py:478-496 (CoCoOp: the vanilla ViT, no prompt rows) -> m->img_f [B, e]
static int vision_forward(mudpt_model* m, const float* images, int B, hipStream_t s) {
    if (m->rn) return resnet_forward(m, images, B, s);  // a handle with the ResNet tower (mudpt_create_frozen_resnet, mudpt_create_resnet)
    const mudpt_config& c = m->cfg;
    const int dv = c.v_width, n = m->vis.n, D1 = m->vis.D1, P = n_patches(c), Lv = m->vis.L, K0 = patch_k0(c);
    const PromptRoute pr = prompt_route(m, m->vis);
    const int m_patch = site_mode(m->vis, SITE_PATCH, K0);  // parity mode: split pixels (an fp16 pixel alone carries 2.4e-4 of rounding into block 0)
    if (m_patch != LO_NONE) TRY(launch_patchify_split(m->dtype, images, m->patches, m->patches_lo, m_patch, B, c.image_size, c.patch, K0, s));
    else TRY(launch_patchify(m->dtype, images, m->patches, B, c.image_size, c.patch, K0, s));
    GemmArgs pe; pe.A = m->patches; pe.lda = K0; pe.B = m->conv_w; pe.ldb = K0; pe.M = B * P; pe.N = dv; pe.K = K0; pe.out0 = m->xpre; pe.ldo0 = dv;
    split_operand(pe, m_patch, m->patches_lo, m->conv_w8, m->conv_s8);
    pe.patches = P; pe.seq_len = Lv; pe.pos = m->vpos;
    TRY(gemm_call(m, EPI_PATCH, pe, s));
    TRY(launch_set_rows(m->xpre, B, Lv, dv, 0, 1, m->cls, m->vpos, s));
    // prompt rows after the positional embedding, before ln_pre
    if (n > 0) TRY(launch_set_rows(m->xpre, B, Lv, dv, Lv - n, n, pr.in0, pr.in0_add, s));
    LnFwdArgs lp; lp.x = m->xpre; lp.ldx = dv; lp.gamma = m->ln_pre_g; lp.beta = m->ln_pre_b; lp.out = m->vis.a[0].x_in; lp.ldo = dv; lp.out_f32 = true;
    lp.mean = m->pre_mean; lp.rstd = m->pre_rstd; lp.rows = B * Lv; lp.d = dv;
    TRY(launch_ln_fwd(m->dtype, lp, s));
    for (int i = 0; i < m->vis.layers; ++i) TRY(block_fwd(m, m->vis, i, B, (i >= 1 && i - 1 < D1) ? pr.deep + (size_t)(i - 1) * n * dv : nullptr, s));
    return tower_head_fwd(m, m->vis, vision_head(m), m->img_f, B, 0, s);
}

// What a forward is given for its image side: the images, for the vision tower, or -- mudpt_forward_features -- the raw [B, e] features that
// tower would leave in m->img_f.  Everything behind m->img_f is one code path for both
struct ImageSide {
    const float *images = nullptr, *features = nullptr;
    ImageSide(const float* images_) : images(images_) {}
    static ImageSide cached(const float* features_) { ImageSide in(nullptr); in.features = features_; return in; }
};
static int image_side_forward(mudpt_model* m, const ImageSide& in, int B, hipStream_t s) {
    if (!in.features) return vision_forward(m, in.images, B, s);
    HIP_TRY(hipMemcpyAsync(m->img_f, in.features, (size_t)B * m->cfg.embed_dim * 4, hipMemcpyDeviceToDevice, s));
    return MUDPT_OK;
}

// One pass of the text tower over nseq sequences of the bound layout, block 0's input in place: the blocks (deep != null: its [D1][n][d] rows spliced
// into blocks 1 .. D1), the head on the EOT rows (statistics rows r0 ..) and, packed, the scatter back to the caller's class order -> feat [nseq, e]
static int text_tower_pass(mudpt_model* m, int nseq, size_t r0, const float* deep, float* feat, hipStream_t s) {
    Tower& X = m->txt;
    for (int i = 0; i < X.layers; ++i) TRY(block_fwd(m, X, i, nseq, (deep && i >= 1 && i - 1 < X.D1) ? deep + (size_t)(i - 1) * X.n * X.d : nullptr, s));
    TRY(tower_head_fwd(m, X, text_head(m), X.packed() ? m->txt_sorted : feat, nseq, r0, s));
    if (X.packed()) TRY(scatter(m->txt_sorted, X.lay->perm, feat, nseq, m->cfg.embed_dim, 4, s));
    return MUDPT_OK;
}

// ---- CoCoOp (trainers/cocoop.py) ------------------------------------------------------------------------------------
// text tower over the prompts of images [i0, i0 + nb): prompts (:148-165) + positional embedding (:52), 12 causal blocks, ln_final on
// the EOT rows, text_projection -> rows i0 * C .. of m->txt_f
static int cocoop_text_chunk(mudpt_model* m, int i0, int nb, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dt = c.t_width, e = c.embed_dim, n = c.n_ctx, C = c.n_cls, Lt = m->txt.L;
    const size_t r0 = (size_t)i0 * C;
    TRY(launch_cocoop_prompts(m->txt.a[0].x_in, m->emb_pos, m->params + m->off(Q_CTX), m->mn_bias + (size_t)i0 * dt, m->tpos, nb, C, Lt, dt, n, s));
    return text_tower_pass(m, nb * C, r0, nullptr, m->txt_f + r0 * e, s);
}

static HeadArgs cocoop_head_args(mudpt_model* m, int i0, int nb, int B) {
    const mudpt_config& c = m->cfg;
    const size_t C = c.n_cls, e = c.embed_dim, r0 = (size_t)i0 * C;
    HeadArgs h; h.img = m->img_f + (size_t)i0 * e; h.txt = m->txt_f + r0 * e; h.scale = m->scale; h.logits = m->logits + r0;
    h.img_n = m->img_n + (size_t)i0 * e; h.txt_n = m->txt_n + r0 * e; h.img_inv = m->img_inv + i0; h.txt_inv = m->txt_inv + r0;
    h.dlogits = m->dlogits + r0; h.row_loss = m->row_loss + i0; h.dtxt = m->dtxt + r0 * e; h.loss = m->loss;
    h.B = nb; h.B_total = B; h.C = (int)C; h.e = (int)e;
    return h;
}

// image features of the frozen vanilla ViT, normalised (:183), and meta_net: linear1 -> ReLU -> linear2 (:103-107, fp32) -> the
// per-image context shift m->mn_bias [B, dt]
static int cocoop_image_side(mudpt_model* m, const ImageSide& in, int B, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dt = c.t_width, e = c.embed_dim, hd = m->hid;
    float* Pm = m->params;
    TRY(image_side_forward(m, in, B, s));
    TRY(launch_l2norm(m->img_f, m->img_n, m->img_inv, B, e, s));
    TRY(launch_sgemm(false, true, B, hd, e, 1.f, m->img_n, e, Pm + m->off(Q_W1), e, 0.f, m->mn_hid, hd, Pm + m->off(Q_B1), s));
    TRY(launch_relu(m->mn_hid, (size_t)B * hd, s));
    TRY(launch_sgemm(false, true, B, dt, hd, 1.f, m->mn_hid, hd, Pm + m->off(Q_W2), hd, 0.f, m->mn_bias, dt, Pm + m->off(Q_B2), s));
    return MUDPT_OK;
}

// forward (:178-198): image features -> meta_net bias per image (:141-146) -> the text tower over the (image, class) prompts, a chunk
// of images per pass (the reference loops image by image, :187-194) -> logits [B, C].
static int cocoop_forward(mudpt_model* m, const ImageSide& in, int B, hipStream_t s) {
    TRY(cocoop_image_side(m, in, B, s));
    for (int i0 = 0; i0 < B; i0 += m->txt_chunk) {
        const int nb = B - i0 < m->txt_chunk ? B - i0 : m->txt_chunk;
        TRY(cocoop_text_chunk(m, i0, nb, s));
        TRY(launch_pair_head_fwd(cocoop_head_args(m, i0, nb, B), s));
    }
    return MUDPT_OK;
}

// forward + F.cross_entropy (:196-197) + backward w.r.t. ctx and meta_net (:222-226 freeze rule: "prompt_learner" only).  Per chunk of
// images: text forward, logits, CE rows, text backward, ctx / bias gradients accumulated in chunk order (fixed: reproducible).
static int cocoop_forward_backward(mudpt_model* m, const float* images, const int64_t* labels, int B, float grad_scale, float* loss, float* logits, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dt = c.t_width, e = c.embed_dim, n = c.n_ctx, C = c.n_cls, Lt = m->txt.L, hd = m->hid;
    float *Pm = m->params, *G = m->grads;
    TRY(cocoop_image_side(m, images, B, s));
    HIP_TRY(hipMemsetAsync(G, 0, m->total * 4, s));
    const float unscale = grad_scale / ((float)B * m->loss_scale);  // static loss scaling, as in mudpt_forward_backward
    Tower& X = m->txt;
    for (int i0 = 0; i0 < B; i0 += m->txt_chunk) {
        const int nb = B - i0 < m->txt_chunk ? B - i0 : m->txt_chunk, TS = nb * C;
        const size_t r0 = (size_t)i0 * C;
        TRY(cocoop_text_chunk(m, i0, nb, s));
        HeadArgs h = cocoop_head_args(m, i0, nb, B);
        h.labels = labels + i0; h.grad_scale = m->loss_scale * (float)B;
        TRY(launch_pair_head_fwd(h, s));
        TRY(launch_pair_head_bwd(h, s));  // CE rows, dlogits, d(text features) of this chunk; the mean over all B rows follows the loop
        TRY(tower_head_bwd(m, X, text_head(m), m->dtxt + r0 * e, TS, r0, s));
        for (int i = X.layers - 1; i >= 0; --i) TRY(block_bwd(m, X, i, TS, s));
        // d ctx += sum over the chunk's (image, class) prompts of the context rows' gradient; d bias[i] = the same sum over image i's prompts
        const GradStream dx = grad_stream(m, X);
        TRY(launch_reduce_rows(m->dtype, dx.f32, dx.lp, TS, Lt, dt, 1, n, G + m->off(Q_CTX), false, true, unscale, s));
        TRY(launch_cocoop_dbias(m->dtype, dx.f32, dx.lp, m->mn_dbias + (size_t)i0 * dt, nb, C, Lt, dt, n, unscale, s));
    }
    TRY(launch_mean(m->row_loss, B, m->loss, s));
    HIP_TRY(hipMemcpyAsync(loss, m->loss, 4, hipMemcpyDeviceToDevice, s));
    if (logits) HIP_TRY(hipMemcpyAsync(logits, m->logits, (size_t)B * C * 4, hipMemcpyDeviceToDevice, s));
    // meta_net backward (fp32, tiny): linear2, ReLU, linear1; its input (the normalised image features) is a constant
    TRY(launch_sgemm(true, false, dt, hd, B, 1.f, m->mn_dbias, dt, m->mn_hid, hd, 0.f, G + m->off(Q_W2), hd, nullptr, s));
    TRY(launch_colsum(m->mn_dbias, B, dt, dt, G + m->off(Q_B2), false, s));
    TRY(launch_sgemm(false, false, B, hd, dt, 1.f, m->mn_dbias, dt, Pm + m->off(Q_W2), hd, 0.f, m->mn_dhid, hd, nullptr, s));
    TRY(launch_relu_bwd(m->mn_dhid, m->mn_hid, (size_t)B * hd, s));
    TRY(launch_sgemm(true, false, hd, e, B, 1.f, m->mn_dhid, hd, m->img_n, e, 0.f, G + m->off(Q_W1), e, nullptr, s));
    TRY(launch_colsum(m->mn_dhid, B, hd, hd, G + m->off(Q_B1), false, s));
    return MUDPT_OK;
}

// ---- the MuDPT step in pieces (the monolithic entry points and the class-parallel phases share them) ------------------------------
// prompt learner, trainers/mudpt.py:117-130 + clip/model.py:534-539
static int prompt_learner_forward(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dv = c.v_width, dt = c.t_width, e = c.embed_dim, n = c.n_ctx, D1 = c.depth - 1;
    float* Pm = m->params;
    TRY(launch_sgemm(false, true, n, dv, dt, 1.f, Pm + m->off(P_CTX), dt, Pm + m->off(P_EW), dt, 0.f, m->shared, dv, Pm + m->off(P_EB), s));
    if (D1 > 0) {
        TRY(launch_sgemm(false, true, D1 * n, dv, dt, 1.f, Pm + m->off(P_DEEP), dt, Pm + m->off(P_DW), dt, 0.f, m->t2v, dv, Pm + m->off(P_DB), s));
        TRY(launch_sgemm(false, true, D1 * n, e, dv, 1.f, Pm + m->off(P_VDEEP), dv, Pm + m->off(P_VW), dv, 0.f, m->v2t, e, Pm + m->off(P_VB), s));
        TRY(launch_add(m->t2v, Pm + m->off(P_VDEEP), m->vis_deep, (size_t)D1 * n * dv, s));
        TRY(launch_add(m->v2t, Pm + m->off(P_DEEP), m->txt_deep, (size_t)D1 * n * dt, s));
    }
    return MUDPT_OK;
}

struct Gen2 {  // UUMuDPT's second generator: depth - 1 layers of n rows, width d = v_width, output width e = embed_dim (= t_width)
    int D1 = 0, n = 0, d = 0, e = 0;
    PgParams P;
    const float* X = nullptr;  // visual_ctx_deep_prompts in the bound parameter bucket
};

// UMuDPT, trainers/umudpt.py:170-176: the vision prompts of every layer from the text prompts of every layer
static int umudpt_forward(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    float* Pm = m->params;
    return pg_forward(c.depth, c.n_ctx, c.t_width, c.v_width, pg_params(Pm + m->off(U_GEN), c.t_width, c.v_width), Pm + m->off(P_CTX), m->pg_G, m->pg_w, s);
}

// UUMuDPT's two directions.  Vision stream: Gen1 as UMuDPT, then the vision deep prompts G[1:] + visual_ctx_deep_prompts (clip/model.py:640).
// Text stream, ahead of the text tower: T = Gen2(visual_ctx_deep_prompts) and the text deep prompts deep_prompts + T (clip/model.py:630-636,
// trainers/uumudpt.py:224).  The two generators share no buffer, so their launch chains run beside each other
static Gen2 uumudpt_gen2(const mudpt_model* m) {
    const mudpt_config& c = m->cfg;
    Gen2 g;
    g.D1 = c.depth - 1; g.n = c.n_ctx; g.d = c.v_width; g.e = c.embed_dim;
    g.P = pg_params(m->params + m->off(UU_GEN2), g.d, g.e);
    g.X = m->params + m->off(UU_VDEEP);
    return g;
}
static int uumudpt_forward_vision(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    TRY(umudpt_forward(m, s));
    const size_t group = (size_t)c.n_ctx * c.v_width, D1 = (size_t)c.depth - 1;
    return D1 > 0 ? launch_add(m->pg_G + group, m->params + m->off(UU_VDEEP), m->vis_deep, D1 * group, s) : MUDPT_OK;
}
static int uumudpt_forward_text(mudpt_model* m, hipStream_t s2) {
    const Gen2 g = uumudpt_gen2(m);
    if (g.D1 <= 0) return MUDPT_OK;
    TRY(pg_forward(g.D1, g.n, g.d, g.e, g.P, g.X, m->pg2_T, m->pg2_w, s2));
    return launch_add(m->params + m->off(P_DEEP), m->pg2_T, m->txt_deep, (size_t)g.D1 * g.n * g.e, s2);
}

// text tower, trainers/mudpt.py:142-156, over this handle's classes [c0, c0 + ct): rows c0.. of the [n_cls, e] feature table
static int text_forward(mudpt_model* m, hipStream_t s2) {
    const mudpt_config& c = m->cfg;
    const int dt = c.t_width, e = c.embed_dim, n = m->txt.n, Ct = m->ct;
    float* Pm = m->params;
    const TowerSegs segs(m->txt, Ct);
    const PromptRoute pr = prompt_route(m, m->txt);
    ++m->text_launches;
    HIP_TRY(hipMemcpyAsync(m->txt.a[0].x_in, m->emb_pos, (size_t)tower_rows(m->txt, Ct) * dt * 4, hipMemcpyDeviceToDevice, s2));
    if (m->coop)  // trainers/coop.py:166-175,187-188: the context rows at every class's own positions, all buckets in one launch
        TRY(launch_coop_splice(m->txt.a[0].x_in, Pm + m->off(0), m->tpos, m->tprompt_rows, m->coop_pos, Ct, n, dt, m->csc, s2));
    else if (n > 0)  // MuDPT ctx / MPT text_prompt_learner.visual_ctx at rows 1..n
        for (const Tower::Seg& g : segs)
            TRY(launch_set_rows(m->txt.a[0].x_in + (size_t)g.row0 * dt, g.nseq, g.L, dt, 1, n, pr.in0, pr.in0_add, s2));
    if (m->sharded) HIP_TRY(hipMemsetAsync(m->txt_f, 0, (size_t)c.n_cls * e * 4, s2));  // other ranks' rows: zero, so a sum completes the table
    TRY(text_tower_pass(m, Ct, 0, pr.deep, m->txt_f + (size_t)m->c0 * e, s2));
    m->text_valid = true;
    return MUDPT_OK;
}

// The variant's trainable front end around the towers, each hook null where the variant has none (learner(), below its last hook):
//   fwd         before the fork: both towers read its output
//   fwd_text    after the fork, on the text stream ahead of the text tower: the vision tower reads none of its output; kept with reuse_text
//   fwd_vision  after the fork, on the vision stream: the text tower reads none of its output, so only the vision tower's prompt splice waits
//               for it; with reuse_text its output is kept like the text features (same parameters, same output)
//   bwd_text    on the text stream behind that tower's backward, before the join: needs the text tower's prompt gradients only
//   bwd         after the join
struct Learner {
    typedef int (*Hook)(mudpt_model*, hipStream_t);
    Hook fwd = nullptr, fwd_text = nullptr, fwd_vision = nullptr, bwd_text = nullptr, bwd = nullptr;
};
static Learner learner(const mudpt_model* m);

// Both towers' forward.  The text tower is independent of the vision tower once the prompt learner has run, so it goes to the side
// stream (enqueued first): its ~200 small launch-latency-bound kernels fill the CUs the big vision kernels leave idle (tails of the
// persistent GEMMs, memory-bound LayerNorms) instead of serialising behind them.  With reuse_text (inference with unchanged
// parameters: the reference recomputes the text tower for every test batch, trainers/mudpt.py:170-184) the text
// features of the previous call are kept.
static int towers_forward(mudpt_model* m, const ImageSide& in, int B, hipStream_t s, bool reuse_text) {
    const Learner L = learner(m);
    m->cl_B = 0;  // every forward overwrites what a mudpt_forward_train left for its backward
    if (L.fwd) TRY(L.fwd(m, s));
    if (!reuse_text) {
        HIP_TRY(hipEventRecord(m->ev_fork, s));
        HIP_TRY(hipStreamWaitEvent(m->s2, m->ev_fork, 0));
        if (L.fwd_text) TRY(L.fwd_text(m, m->s2));
        TRY(text_forward(m, m->s2));
        HIP_TRY(hipEventRecord(m->ev_join, m->s2));
        if (L.fwd_vision) TRY(L.fwd_vision(m, s));
    }
    TRY(image_side_forward(m, in, B, s));  // clip/model.py:526-553
    if (!reuse_text) HIP_TRY(hipStreamWaitEvent(s, m->ev_join, 0));
    return MUDPT_OK;
}

// cosine logits, trainers/mudpt.py:178-182 (needs both towers' features; txt_f must hold all n_cls rows)
static int head_forward(mudpt_model* m, int B, bool reuse_text, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    m->cl_B = 0;
    HeadArgs h; h.img = m->img_f; h.txt = m->txt_f; h.scale = m->scale; h.logits = m->logits; h.img_n = m->img_n; h.txt_n = m->txt_n;
    h.img_inv = m->img_inv; h.txt_inv = m->txt_inv; h.B = B; h.C = c.n_cls; h.e = c.embed_dim;
    if (!reuse_text || !head_fused_fits(h, false)) ++m->text_launches;  // the normalisation of the text features
    if (head_fused_fits(h, false)) {
        if (reuse_text) h.txt = nullptr;  // the normalised text features of the previous call are still in m->txt_n
        TRY(launch_head_fused_fwd(h, s));
    } else {
        TRY(launch_head_fwd(h, s));
    }
    return MUDPT_OK;
}

static int forward_impl(mudpt_model* m, const ImageSide& in, int B, hipStream_t s, bool reuse_text = false, bool skip_head = false) {
    if (m->cocoop) return cocoop_forward(m, in, B, s);
    TRY(towers_forward(m, in, B, s, reuse_text));
    if (skip_head) return MUDPT_OK;  // the training step runs the fused forward + cross-entropy + backward head itself
    return head_forward(m, B, reuse_text, s);
}

// ---- frozen CLIP (trainers/zsclip.py) ------------------------------------------------------------------------------------
static int frozen_ready(mudpt_model* m, const char* what, int B, bool need_text, bool need_vision = true) {
    ARG_CHECK(m, "%s: null model", what);
    ARG_CHECK(m->frozen, "%s: not a frozen handle (mudpt_create_frozen)", what);
    for (const std::string& k : m->missing)  // the image side needs the vision tower's weights only, a forward from cached features none of them
        if (k.rfind("visual.", 0) == 0 ? need_vision : need_text) { set_error("%s: model not ready: %zu frozen weights unset (first needed: %s)", what, m->missing.size(), k.c_str()); return MUDPT_ERR_STATE; }
    if (need_text && !m->prompts_set) { set_error("%s: model not ready: call mudpt_set_text_tokens", what); return MUDPT_ERR_STATE; }
    ARG_CHECK(B > 0 && B <= m->cfg.max_batch, "%s: batch %d outside 1..max_batch=%d", what, B, m->cfg.max_batch);
    return MUDPT_OK;
}

// The text features of a frozen handle -> m->txt_n [n_cls, e], rows of norm 1.  Templates in ascending order, each: block 0's input from the token
// ids (zeroshot.hip; no emb_pos copy), the text tower and its head on the EOT rows (clip/model.py:825-838), the bucket scatter back to the
// caller's class order, the ensemble step (zsclip.py:67-71 one template, :107-117 more).  A template has n_cls >= 1 sequences of >= 2 rows: no
// launch here has zero rows.  The order is fixed and every kernel's sums are: two builds agree bit for bit.
static int frozen_text_features(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dt = c.t_width, e = c.embed_dim, C = c.n_cls, T = (int)m->tmpl.size();
    Tower& X = m->txt;
    for (int t = 0; t < T; ++t) {
        const mudpt_model::Template& P = m->tmpl[t];
        bind_text_layout(X, P.lay);
        ++m->text_launches;
        TRY(launch_embed_tokens(m->tok_table, m->vocab, P.tok, P.pos, m->tpos, X.a[0].x_in, P.lay.rows, dt, s));
        TRY(text_tower_pass(m, C, 0, nullptr, m->txt_f, s));
        TRY(launch_feature_ensemble(m->txt_f, m->ens_acc, m->txt_n, C, e, t == 0, t == T - 1, T, s));
    }
    m->text_valid = true;
    return MUDPT_OK;
}

// model_inference (zsclip.py:74-79): the vanilla vision tower, then the logits-only head against the kept table (the head never
// re-normalises it: a.txt = null).  Inference: never a split K
static int frozen_forward(mudpt_model* m, const ImageSide& in, int B, float* logits, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    if (!m->text_valid) TRY(frozen_text_features(m, s));
    m->train_fwd = false;
    TRY(image_side_forward(m, in, B, s));
    HeadArgs h; h.img = m->img_f; h.scale = m->scale; h.logits = m->logits; h.img_n = m->img_n; h.txt_n = m->txt_n;
    h.img_inv = m->img_inv; h.txt_inv = m->txt_inv; h.B = B; h.C = c.n_cls; h.e = c.embed_dim;
    if (head_fused_fits(h, false)) {
        TRY(launch_head_fused_fwd(h, s));
    } else {
        TRY(launch_l2norm(m->img_f, m->img_n, m->img_inv, B, c.embed_dim, s));
        TRY(launch_sgemm(false, true, B, c.n_cls, c.embed_dim, m->scale, m->img_n, c.embed_dim, m->txt_n, c.embed_dim, 0.f, m->logits, c.n_cls, nullptr, s));
    }
    HIP_TRY(hipMemcpyAsync(logits, m->logits, (size_t)B * c.n_cls * 4, hipMemcpyDeviceToDevice, s));
    return MUDPT_OK;
}

extern "C" int mudpt_text_features(mudpt_model* m, float* feat, void* stream) {
    TRY(frozen_ready(m, "text_features", 1, true, false));  // the text side alone: a handle that serves cached image features has no visual.* weights
    ARG_CHECK(feat, "text_features: null argument");
    hipStream_t s = (hipStream_t)stream;
    if (!m->text_valid) TRY(frozen_text_features(m, s));
    HIP_TRY(hipMemcpyAsync(feat, m->txt_n, (size_t)m->cfg.n_cls * m->cfg.embed_dim * 4, hipMemcpyDeviceToDevice, s));
    return MUDPT_OK;
}

// clip/model.py:822 encode_image, lpclip/feat_extractor.py:125: the raw features, as the vision tower's projection leaves them
extern "C" int mudpt_encode_image(mudpt_model* m, const float* images, int32_t B, float* features, void* stream) {
    TRY(frozen_ready(m, "encode_image", B, false));
    ARG_CHECK(images && features, "encode_image: null argument");
    hipStream_t s = (hipStream_t)stream;
    m->train_fwd = false;
    m->feat_B = 0;
    TRY(vision_forward(m, images, B, s));
    HIP_TRY(hipMemcpyAsync(features, m->img_f, (size_t)B * m->cfg.embed_dim * 4, hipMemcpyDeviceToDevice, s));
    m->feat_B = B;
    return MUDPT_OK;
}

static int not_sharded(mudpt_model* m, const char* what) {
    if (m->sharded) { set_error("%s: this handle encodes classes %d..%d of %d only (mudpt_set_class_shard): use the mudpt_cp_* phases", what, m->c0, m->c0 + m->ct - 1, m->cfg.n_cls); return MUDPT_ERR_STATE; }
    return MUDPT_OK;
}

extern "C" int mudpt_forward(mudpt_model* m, const float* images, int32_t B, float* logits, void* stream) {
    return mudpt_forward_ex(m, images, B, logits, 0, stream);
}

static const char* variant_name(const mudpt_model* m) {
    return m->frozen ? "frozen CLIP" : m->cocoop ? "CoCoOp" : m->coop ? "CoOp" : m->vpt ? "VPT" : m->mpt ? "MPT" : m->uumudpt ? "UUMuDPT" : m->umudpt ? "UMuDPT" : "MuDPT";
}
// The handles whose visual(image) is a constant of the image: the frozen, prompt-free tower of trainers/zsclip.py:74-79, coop.py:212-223 and
// cocoop.py:178-188.  The other five splice trainable prompts into the vision tower (MPT: it may; its handle is refused whole)
static int features_are_constant(const mudpt_model* m, const char* what) {
    ARG_CHECK(m, "%s: null model", what);
    ARG_CHECK(m->frozen || m->coop || m->cocoop, "%s: refused for %s: its trainable prompts run inside the vision tower, so its image features are no constant "
              "of the image and cannot be cached; run mudpt_forward on the images", what, variant_name(m));
    return MUDPT_OK;
}

// One inference forward (mudpt_forward_ex: what = "forward", from the images; mudpt_forward_features: from the features): every check, then
// the launches.  A call that fails a check has launched nothing and changed nothing
static int inference_forward(mudpt_model* m, const ImageSide& in, int32_t B, float* logits, int32_t flags, void* stream, const char* what) {
    const bool cached = in.features != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (m && m->frozen) {  // MUDPT_FWD_REUSE_TEXT changes nothing: the text features are kept anyway
        TRY(frozen_ready(m, what, B, true, !cached));
        ARG_CHECK((in.images || in.features) && logits, "%s: null argument", what);
        m->feat_B = 0;
        TRY(frozen_forward(m, in, B, logits, s));
        m->feat_B = B;
        return MUDPT_OK;
    }
    TRY(ready(m, B, false));
    TRY(not_sharded(m, what));
    ARG_CHECK((in.images || in.features) && logits, "%s: null argument", what);
    // CoCoOp's text features depend on the image; VPT's on nothing trainable: once computed they stay (until mudpt_set_weight / _set_class_prompts)
    const bool reuse = ((flags & MUDPT_FWD_REUSE_TEXT) != 0 || (m->vpt && m->text_valid)) && !m->cocoop;
    if (reuse && !m->text_valid) { set_error("%s: MUDPT_FWD_REUSE_TEXT before any text-tower pass", what); return MUDPT_ERR_STATE; }
    m->train_fwd = false;
    m->feat_B = 0;
    TRY(forward_impl(m, in, B, s, reuse));
    HIP_TRY(hipMemcpyAsync(logits, m->logits, (size_t)B * m->cfg.n_cls * 4, hipMemcpyDeviceToDevice, s));
    m->feat_B = B;
    return MUDPT_OK;
}

extern "C" int mudpt_forward_ex(mudpt_model* m, const float* images, int32_t B, float* logits, int32_t flags, void* stream) {
    return inference_forward(m, ImageSide(images), B, logits, flags, stream, "forward");
}

// model_inference behind clip_model.visual(image) (trainers/zsclip.py:76-79, coop.py:214-223, cocoop.py:182-198): the forward above from the
// features lpclip/feat_extractor.py:125 saves
extern "C" int mudpt_forward_features(mudpt_model* m, const float* features, int32_t B, float* logits, int32_t flags, void* stream) {
    TRY(features_are_constant(m, "forward_features"));
    ARG_CHECK(features, "forward_features: null argument");
    return inference_forward(m, ImageSide::cached(features), B, logits, flags, stream, "forward_features");
}

// lpclip/feat_extractor.py:125: visual(image) of the batch the last inference forward ran on
extern "C" int mudpt_image_features(mudpt_model* m, int32_t B, float* features, void* stream) {
    TRY(features_are_constant(m, "image_features"));
    ARG_CHECK(features, "image_features: null argument");
    if (m->feat_B == 0) { set_error("image_features: no inference forward since the handle was created or since its last training step"); return MUDPT_ERR_STATE; }
    if (m->feat_B != B) { set_error("image_features: the last inference forward ran on %d images, not %d", m->feat_B, B); return MUDPT_ERR_STATE; }
    HIP_TRY(hipMemcpyAsync(features, m->img_f, (size_t)B * m->cfg.embed_dim * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MUDPT_OK;
}

// head of the training step: cross-entropy (mean) + cosine logits backward, trainers/mudpt.py:178-182,250 -> loss, dimg, dtxt (all classes)
// reuse_text (VPT): m->txt_n / txt_inv still hold the normalised features of the cached text pass; text_grad = false (VPT): no dtxt
// A ResNet handle (CoOp on mudpt_create_resnet) asks for no dimg: nothing in front of its image features trains, and without the gradient tile
// the fused head takes embed_dim 1024 up to 1520 classes (with it: 496).  ViT handles keep passing m->dimg, CoOp's included
static int head_train(mudpt_model* m, const int64_t* labels, int B, float grad_scale, float* loss, float* logits, hipStream_t s,
                      bool reuse_text = false, bool text_grad = true) {
    const mudpt_config& c = m->cfg;
    const int e = c.embed_dim, C = c.n_cls;
    m->cl_B = 0;
    HeadArgs h; h.img = m->img_f; h.txt = m->txt_f; h.labels = labels; h.scale = m->scale; h.logits = m->logits; h.loss = m->loss; h.dlogits = m->dlogits;
    h.row_loss = m->row_loss; h.dimg = m->rn ? nullptr : m->dimg; h.dtxt = text_grad ? m->dtxt : nullptr; h.img_n = m->img_n; h.txt_n = m->txt_n; h.img_inv = m->img_inv; h.txt_inv = m->txt_inv;
    // Static loss scaling: the backward pass runs on per-sample gradients times loss_scale (dlogits = (softmax -
    // onehot) * loss_scale, independent of B and of the number of ranks), so the T copies of the token gradients
    // stay inside fp16's normal range (unscaled they are ~1e-7 at B = 256: flushed).  Every reduction that leaves a
    // tower multiplies by `unscale` = grad_scale / (B * loss_scale); everything after them (prompt-learner and generator
    // backwards, meta_net, the bucket) is fp32 and linear.  The sites (tests/test_scales_gpu.py runs each):
    //   text_backward    launch_reduce_rows per length bucket and deep layer, and again per bucket for layer 0's prompt rows;
    //                    CoOp: launch_coop_dctx instead (shared or per-class context)
    //   vision_backward  launch_reduce_rows per deep layer, once over the fused splice (vsplice), once for layer 0's prompt rows
    //   cocoop_forward_backward  launch_reduce_rows (d ctx) and launch_cocoop_dbias, per chunk of images, with an unscale of its own
    //   the class-parallel phases  mudpt_cp_backward passes the cp_unscale that the step's mudpt_cp_head stored here
    m->cp_unscale = grad_scale / ((float)B * m->loss_scale);
    h.grad_scale = m->loss_scale * (float)B; h.B = B; h.C = C; h.e = e;
    if (text_grad) ++m->text_launches;  // the text half of the backward (head_dtxt_kernel / its unfused form)
    if (head_fused_fits(h, true)) {
        if (reuse_text) h.txt = nullptr;  // keep the normalised text features
        else ++m->text_launches;
        TRY(launch_head_fused_train(h, s));
    } else {
        TRY(head_forward(m, B, reuse_text, s));
        TRY(launch_head_bwd(h, s));
    }
    if (logits) HIP_TRY(hipMemcpyAsync(logits, m->logits, (size_t)B * C * 4, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(loss, m->loss, 4, hipMemcpyDeviceToDevice, s));
    return MUDPT_OK;
}

// text tower backward over this handle's classes: reads rows c0.. of dtxt and its own activations, writes only its own buffers,
// d_txt_deep and the ctx slice of the gradient bucket
static int text_backward(mudpt_model* m, float unscale, hipStream_t s2) {
    const mudpt_config& c = m->cfg;
    const int dt = c.t_width, e = c.embed_dim, n = m->txt.n, D1 = m->txt.D1, Ct = m->ct;
    float* G = m->grads;
    Tower& X = m->txt;
    const PromptRoute pr = prompt_route(m, X);
    ++m->text_launches;
    const TowerSegs segs(X, Ct);
    const float* dfeat = m->dtxt + (size_t)m->c0 * e;
    if (X.packed()) {  // length buckets: the tower's sequences are in length-sorted order
        TRY(gather(dfeat, m->lay.perm, m->dtxt_sorted, Ct, e, 4, s2));
        dfeat = m->dtxt_sorted;
    }
    TRY(tower_head_bwd(m, X, text_head(m), dfeat, Ct, 0, s2));
    for (int i = X.layers - 1; i >= 0; --i) {
        TRY(block_bwd(m, X, i, Ct, s2));
        // zero_src: the T copy is passed in both modes, since it is the copy block i - 1's dX GEMMs read and must see the zeros too
        if (i >= 1 && i - 1 < D1)
            for (const Tower::Seg& g : segs)  // bucket after bucket in a fixed order: deterministic
                TRY(launch_reduce_rows(m->dtype, grad_stream(m, X, g.row0).f32, lp_at(X.dx_lp, (size_t)g.row0 * dt), g.nseq, g.L, dt, 1, n,
                                       pr.d_deep + (size_t)(i - 1) * n * dt, true, g.seq0 > 0, unscale, s2));
    }
    // CoOp: d ctx from the context rows of every class (shared: summed over the classes in a fixed order; CSC: per class), coop.hip
    if (m->coop) return launch_coop_dctx(m->dtype, grad_stream(m, X).f32, grad_stream(m, X).lp, m->tprompt_rows, G + m->off(0), Ct, n, dt, m->csc, unscale, s2);
    // d ctx (text side): rows 1..n of the first block's input, summed over the class prompts
    for (const Tower::Seg& g : segs)
        TRY(launch_reduce_rows(m->dtype, grad_stream(m, X, g.row0).f32, grad_stream(m, X, g.row0).lp, g.nseq, g.L, dt, 1, n, pr.d_in0, false, true, unscale, s2));
    return MUDPT_OK;
}

static int vision_backward(mudpt_model* m, int B, float unscale, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dv = c.v_width, n = m->vis.n, D1 = m->vis.D1, Lv = m->vis.L;
    Tower& V = m->vis;
    const PromptRoute pr = prompt_route(m, V);
    TRY(tower_head_bwd(m, V, vision_head(m), m->dimg, B, 0, s));
    // Backward of the splice: the prompt rows of d(x_in[i]) feed d(vis_deep[i-1]) and the rows the splice overwrote get no gradient.
    // ln_1's backward writes those rows, in fp32, to vsplice[b][(i - 1) n + k][:] and zeros to the stream (LnBwdArgs::side); ONE
    // fixed-order reduction over the images after the last block replaces a reduce-and-zero launch per block on the critical path.
    const int used = used_prompt_rows(V, D1);
    const size_t side_ldb = (size_t)used * dv;
    for (int i = V.layers - 1; i >= 0; --i) {
        const bool spliced = i >= 1 && i - 1 < D1;
        TRY(block_bwd(m, V, i, B, s, spliced ? m->vsplice + (size_t)(i - 1) * n * dv : nullptr, side_ldb));
        // the tail's ln_1 backward is not fused: take the rows from the stream (zero_src: the T copy in both modes, as in text_backward)
        if (spliced && i == V.layers - 1)
            TRY(launch_reduce_rows(m->dtype, grad_stream(m, V).f32, V.dx_lp, B, Lv, dv, Lv - n, n, pr.d_deep + (size_t)(i - 1) * n * dv, true, false, unscale, s));
    }
    // blocks 1 .. layers-2 (the fused ones): rows 0 .. n (layers - 2) of every image's side block
    const int fused = (V.layers - 2 < D1 ? V.layers - 2 : D1) * n;
    if (fused > 0) TRY(launch_reduce_rows(m->dtype, m->vsplice, nullptr, B, used, dv, 0, fused, pr.d_deep, false, false, unscale, s));
    // ln_pre backward on the prompt rows only (patch / CLS rows have no trainable ancestor), in place
    LnBwdArgs bp; bp.dy = m->lp_grad ? (const void*)V.dx_lp : (const void*)V.dx; bp.lddy = dv; bp.dy_f32 = !m->lp_grad; bp.x = m->xpre; bp.ldx = dv; bp.row_index = m->vprompt_rows; bp.mean = m->pre_mean; bp.rstd = m->pre_rstd;
    bp.gamma = m->ln_pre_g; bp.dx = V.dx; bp.lddx = dv; bp.rows = B * n; bp.d = dv; bp.by_token = true;
    TRY(launch_ln_bwd(m->dtype, bp, s));
    TRY(launch_reduce_rows(m->dtype, V.dx, nullptr, B, Lv, dv, Lv - n, n, pr.d_in0, false, false, unscale, s));
    return MUDPT_OK;
}

// prompt learner backward (fp32, tiny), in two halves: the one that needs only the TEXT tower's prompt gradients is enqueued on the text
// stream behind that tower's backward, where it overlaps the vision tower's (round 4: 5 of the 15 tiny launches leave the step's serial
// tail); the other half runs after the join.  Every gradient tensor the halves share is a sum of two terms, one from each: fp32 addition
// of two terms does not depend on which comes first, so the result is bit-identical to the one-stream order.
static int prompt_learner_backward_text(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dv = c.v_width, dt = c.t_width, e = c.embed_dim, n = c.n_ctx, D1 = c.depth - 1;
    float *Pm = m->params, *G = m->grads;
    if (D1 <= 0) return MUDPT_OK;
    const int R = D1 * n;
    TRY(zero_unused_rows(m->d_txt_deep, used_prompt_rows(m->txt, D1), R, dt, s));
    // txt_deep = deep_prompts + visual_ctx_deep_projections(visual_ctx_deep_prompts)   (mudpt.py:175, clip/model.py:539)
    TRY(launch_add(G + m->off(P_DEEP), m->d_txt_deep, G + m->off(P_DEEP), (size_t)R * dt, s));
    TRY(launch_sgemm(true, false, e, dv, R, 1.f, m->d_txt_deep, e, Pm + m->off(P_VDEEP), dv, 1.f, G + m->off(P_VW), dv, nullptr, s));
    TRY(launch_colsum(m->d_txt_deep, R, e, e, G + m->off(P_VB), true, s));
    TRY(launch_sgemm(false, false, R, dv, e, 1.f, m->d_txt_deep, e, Pm + m->off(P_VW), dv, 1.f, G + m->off(P_VDEEP), dv, nullptr, s));
    return MUDPT_OK;
}
static int prompt_learner_backward_vision(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dv = c.v_width, dt = c.t_width, n = c.n_ctx, D1 = c.depth - 1;
    float *Pm = m->params, *G = m->grads;
    // visual_ctx and shared = embed_projection(ctx) both receive d_vprompt0 (clip/model.py:534)
    TRY(launch_add(G + m->off(P_VCTX), m->d_vprompt0, G + m->off(P_VCTX), (size_t)n * dv, s));
    TRY(launch_sgemm(true, false, dv, dt, n, 1.f, m->d_vprompt0, dv, Pm + m->off(P_CTX), dt, 1.f, G + m->off(P_EW), dt, nullptr, s));
    TRY(launch_colsum(m->d_vprompt0, n, dv, dv, G + m->off(P_EB), true, s));
    TRY(launch_sgemm(false, false, n, dt, dv, 1.f, m->d_vprompt0, dv, Pm + m->off(P_EW), dt, 1.f, G + m->off(P_CTX), dt, nullptr, s));
    if (D1 > 0) {
        const int R = D1 * n;
        TRY(zero_unused_rows(m->d_vis_deep, used_prompt_rows(m->vis, D1), R, dv, s));
        // vis_deep = deep_projections(deep_prompts) + visual_ctx_deep_prompts   (clip/model.py:537, mudpt.py:127)
        TRY(launch_add(G + m->off(P_VDEEP), m->d_vis_deep, G + m->off(P_VDEEP), (size_t)R * dv, s));
        TRY(launch_sgemm(true, false, dv, dt, R, 1.f, m->d_vis_deep, dv, Pm + m->off(P_DEEP), dt, 1.f, G + m->off(P_DW), dt, nullptr, s));
        TRY(launch_colsum(m->d_vis_deep, R, dv, dv, G + m->off(P_DB), true, s));
        TRY(launch_sgemm(false, false, R, dt, dv, 1.f, m->d_vis_deep, dv, Pm + m->off(P_DW), dt, 1.f, G + m->off(P_DEEP), dt, nullptr, s));
    }
    return MUDPT_OK;
}
static int prompt_learner_backward(mudpt_model* m, hipStream_t s) {  // both halves on one stream (the class-parallel phases)
    TRY(prompt_learner_backward_text(m, s));
    return prompt_learner_backward_vision(m, s);
}

// UMuDPT: the generator's backward, behind the vision tower's (which leaves dG) and the join with the text stream.  The text tower's backward
// has by then added d_txt_deep into grad(deep_prompts) and the text-input gradient of rows 1..n into grad(ctx), both from zero; dX is the
// second and last term of either tensor, so the sums are bit-identical to any other order of the two (the argument above).
static int umudpt_backward(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    const int dv = c.v_width, dt = c.t_width, n = c.n_ctx, R = c.depth * n;
    float *Pm = m->params, *G = m->grads;
    TRY(zero_unused_rows(m->pg_dG, n + used_prompt_rows(m->vis, c.depth - 1), R, dv, s));  // row group 0: the input prompt rows
    TRY(pg_backward(c.depth, n, dt, dv, pg_params(Pm + m->off(U_GEN), dt, dv), Pm + m->off(P_CTX), m->pg_dG, m->pg_dX, G + m->off(U_GEN), m->pg_w, s));
    return launch_add(G + m->off(P_CTX), m->pg_dX, G + m->off(P_CTX), (size_t)R * dt, s);  // ctx and deep_prompts lie one behind the other
}

// UUMuDPT.  Text stream, behind the text tower's backward (which reduced dT = d_txt_deep and, into the zeroed bucket, grad(ctx)): grad(deep_prompts)
// takes dT as its first term, Gen2's backward WRITES its 18 gradients and, as dX, the first term of grad(visual_ctx_deep_prompts).  After the
// join: Gen1's backward as UMuDPT (the second term of grad(ctx | deep_prompts)), then dG, the vision tower's term, onto
// grad(visual_ctx | visual_ctx_deep_prompts), which lie one behind the other.  Every shared tensor gets exactly two fp32 terms, one per stream
// and the second after the join: bit-identical to any order of the two.  Depth 1: Gen2's gradients stay the zeroed bucket's zeros.
static int uumudpt_backward_text(mudpt_model* m, hipStream_t s2) {
    const Gen2 g = uumudpt_gen2(m);
    if (g.D1 <= 0) return MUDPT_OK;
    float* G = m->grads;
    const int R = g.D1 * g.n;
    TRY(zero_unused_rows(m->d_txt_deep, used_prompt_rows(m->txt, g.D1), R, g.e, s2));
    TRY(launch_add(G + m->off(P_DEEP), m->d_txt_deep, G + m->off(P_DEEP), (size_t)R * g.e, s2));
    return pg_backward(g.D1, g.n, g.d, g.e, g.P, g.X, m->d_txt_deep, G + m->off(UU_VDEEP), G + m->off(UU_GEN2), m->pg2_w, s2);
}
static int uumudpt_backward(mudpt_model* m, hipStream_t s) {
    const mudpt_config& c = m->cfg;
    float* G = m->grads;
    TRY(umudpt_backward(m, s));
    return launch_add(G + m->off(UU_VCTX), m->pg_dG, G + m->off(UU_VCTX), (size_t)c.depth * c.n_ctx * c.v_width, s);
}

// The one place a variant names its learner: CoOp / VPT / MPT have none, their trainables go into the towers as they are
// (trainers/coop.py:166-175); CoCoOp's meta_net is part of its own step
static Learner learner(const mudpt_model* m) {
    Learner L;
    if (m->uumudpt) { L.fwd_text = uumudpt_forward_text; L.fwd_vision = uumudpt_forward_vision; L.bwd_text = uumudpt_backward_text; L.bwd = uumudpt_backward; }
    else if (m->umudpt) { L.fwd_vision = umudpt_forward; L.bwd = umudpt_backward; }
    else if (!m->cocoop && !m->coop && !m->indep) { L.fwd = prompt_learner_forward; L.bwd_text = prompt_learner_backward_text; L.bwd = prompt_learner_backward_vision; }
    return L;
}

// One training step of every variant but CoCoOp: forward, cross-entropy, the backward of each tower that has a trainable ancestor, the
// learner's backward.  VPT (trainers/vpt.py:168-200): the text tower runs on the first step only (its features depend on no trainable), the
// head skips its text half, and the step is vision forward, head and vision backward.  A vanilla vision tower (CoOp, trainers/coop.py:281-296;
// MPT without a vision prompt, mpt.py:224-256): the text tower's backward alone, on the main stream.
extern "C" int mudpt_forward_backward(mudpt_model* m, const float* images, const int64_t* labels, int32_t B, float grad_scale,
                                      float* loss, float* logits, void* stream) {
    NOT_FROZEN(m, "forward_backward");
    TRY(ready(m, B, true));
    ARG_CHECK(images && labels && loss, "forward_backward: null argument");
    hipStream_t s = (hipStream_t)stream;
    m->train_fwd = true;
    m->feat_B = 0;  // a training forward may split K: its features are not the ones a test pass caches
    if (m->cocoop) return cocoop_forward_backward(m, images, labels, B, grad_scale, loss, logits, s);
    TRY(not_sharded(m, "forward_backward"));
    const Learner L = learner(m);
    const bool reuse = m->vpt && m->text_valid;
    TRY(towers_forward(m, images, B, s, reuse));
    HIP_TRY(hipMemsetAsync(m->grads, 0, m->total * 4, s));
    TRY(head_train(m, labels, B, grad_scale, loss, logits, s, reuse, !m->vpt));
    if (m->vpt) return vision_backward(m, B, m->cp_unscale, s);
    if (!m->vis.head_rows) return text_backward(m, m->cp_unscale, s);
    // text tower backward on the side stream (enqueued first; joins before the learner's backward)
    HIP_TRY(hipEventRecord(m->ev_fork_b, s));
    HIP_TRY(hipStreamWaitEvent(m->s2, m->ev_fork_b, 0));
    TRY(text_backward(m, m->cp_unscale, m->s2));
    if (L.bwd_text) TRY(L.bwd_text(m, m->s2));
    HIP_TRY(hipEventRecord(m->ev_join_b, m->s2));
    TRY(vision_backward(m, B, m->cp_unscale, s));
    HIP_TRY(hipStreamWaitEvent(s, m->ev_join_b, 0));
    return L.bwd ? L.bwd(m, s) : MUDPT_OK;
}

// ---- the step split at the head: a loss of the caller's (mudpt_forward_train -> the caller's loss -> mudpt_backward_logits) ----
// One training forward leaves the towers' activations and the head's state (img_n, img_inv, txt_n, txt_inv) in place; the backward starts from
// the caller's dL/dlogits, dL/d(image features), dL/d(text features) instead of from labels and then runs the tail of mudpt_forward_backward.
static int custom_loss_ok(const mudpt_model* m, const char* what) {
    ARG_CHECK(m, "%s: null model", what);
    ARG_CHECK(!m->frozen, "%s: a frozen handle (mudpt_create_frozen) has no parameters: nothing to train with a custom loss", what);
    ARG_CHECK(!m->sharded, "%s: a class-sharded handle (mudpt_set_class_shard) has no custom-loss step: its logits exist only behind the mudpt_cp_* exchanges", what);
    ARG_CHECK(!m->cocoop, "%s: CoCoOp has no custom-loss step: its step is chunked over the images and frees each chunk's text activations before "
              "the next, so all logits exist only after every backward would have had to start", what);
    return MUDPT_OK;
}
static int custom_loss_armed(const mudpt_model* m, int B, const char* what) {
    if (m->cl_B == 0) { set_error("%s: no mudpt_forward_train is in flight: one forward feeds one backward, and any other forward, step or a second backward ends it", what); return MUDPT_ERR_STATE; }
    if (m->cl_B != B) { set_error("%s: the mudpt_forward_train in flight ran on %d images, not %d: one forward feeds one backward of the same batch", what, m->cl_B, B); return MUDPT_ERR_STATE; }
    return MUDPT_OK;
}

extern "C" int mudpt_forward_train(mudpt_model* m, const float* images, int32_t B, float* logits, void* stream) {
    TRY(custom_loss_ok(m, "forward_train"));
    TRY(ready(m, B, true));
    ARG_CHECK(images && logits, "forward_train: null argument");
    hipStream_t s = (hipStream_t)stream;
    m->train_fwd = true;
    m->feat_B = 0;  // as mudpt_forward_backward: a training forward may split K
    m->cp_stage = 0;
    const bool reuse = m->vpt && m->text_valid;
    TRY(towers_forward(m, images, B, s, reuse));
    TRY(head_forward(m, B, reuse, s));
    HIP_TRY(hipMemcpyAsync(logits, m->logits, (size_t)B * m->cfg.n_cls * 4, hipMemcpyDeviceToDevice, s));
    m->cl_B = B;
    ++m->cl_serial;
    return MUDPT_OK;
}

extern "C" int mudpt_train_token(mudpt_model* m, int64_t expect, int64_t* token) {
    TRY(custom_loss_ok(m, "train_token"));
    if (m->cl_B == 0) { set_error("train_token: no mudpt_forward_train is in flight: one forward feeds one backward, and any other forward, step or a second backward ends it"); return MUDPT_ERR_STATE; }
    if (expect != 0 && expect != m->cl_serial) {
        set_error("train_token: the mudpt_forward_train in flight is number %lld of this handle, not %lld: a later forward has overwritten what that one left: "
                  "one forward feeds one backward, and any other forward ends it", (long long)m->cl_serial, (long long)expect);
        return MUDPT_ERR_STATE;
    }
    if (token) *token = m->cl_serial;
    return MUDPT_OK;
}

extern "C" int mudpt_train_release(mudpt_model* m) {
    ARG_CHECK(m, "train_release: null model");
    m->cl_B = 0;
    return MUDPT_OK;
}

extern "C" int mudpt_train_features(mudpt_model* m, int32_t B, float* image_features, float* text_features, void* stream) {
    TRY(custom_loss_ok(m, "train_features"));
    TRY(custom_loss_armed(m, B, "train_features"));
    hipStream_t s = (hipStream_t)stream;
    const size_t e = (size_t)m->cfg.embed_dim;
    if (image_features) HIP_TRY(hipMemcpyAsync(image_features, m->img_f, (size_t)B * e * 4, hipMemcpyDeviceToDevice, s));
    if (text_features) HIP_TRY(hipMemcpyAsync(text_features, m->txt_f, (size_t)m->cfg.n_cls * e * 4, hipMemcpyDeviceToDevice, s));
    return MUDPT_OK;
}

extern "C" int mudpt_backward_logits(mudpt_model* m, const float* dlogits, const float* dimg, const float* dtxt, int32_t B, float grad_scale, void* stream) {
    TRY(custom_loss_ok(m, "backward_logits"));
    TRY(ready(m, B, true));
    ARG_CHECK(dlogits || dimg || dtxt, "backward_logits: dlogits, dimg and dtxt are all null: no gradient to start from");
    TRY(custom_loss_armed(m, B, "backward_logits"));
    m->cl_B = 0;  // consumed, whatever happens below
    hipStream_t s = (hipStream_t)stream;
    const mudpt_config& c = m->cfg;
    const Learner L = learner(m);
    HIP_TRY(hipMemsetAsync(m->grads, 0, m->total * 4, s));
    const bool img_grad = !m->rn && m->vis.head_rows, txt_grad = !m->vpt;  // the towers with a trainable ancestor, as mudpt_forward_backward's shortcuts
    const float gmul = m->loss_scale * (float)B;  // the convention of head_train: per-sample gradients times loss_scale inside the towers
    m->cp_unscale = grad_scale / gmul;
    HeadGradArgs h; h.img_n = m->img_n; h.img_inv = m->img_inv; h.txt_n = m->txt_n; h.txt_inv = m->txt_inv; h.G = dlogits; h.ldg = c.n_cls;
    h.Eimg = img_grad ? dimg : nullptr; h.Etxt = txt_grad ? dtxt : nullptr; h.dimg = img_grad ? m->dimg : nullptr; h.dtxt = txt_grad ? m->dtxt : nullptr;
    h.scale = m->scale; h.gmul = gmul; h.B = B; h.C = c.n_cls; h.e = c.embed_dim;
    if (!h.G && !h.Eimg && !h.Etxt) return MUDPT_OK;  // only gradients of features nothing trainable stands in front of: the bucket stays zero
    if (txt_grad) ++m->text_launches;  // the text half of the head's backward, as head_train counts it
    TRY(launch_head_grad(h, s));
    if (m->vpt) return vision_backward(m, B, m->cp_unscale, s);
    if (!m->vis.head_rows) return text_backward(m, m->cp_unscale, s);
    HIP_TRY(hipEventRecord(m->ev_fork_b, s));
    HIP_TRY(hipStreamWaitEvent(m->s2, m->ev_fork_b, 0));
    TRY(text_backward(m, m->cp_unscale, m->s2));
    if (L.bwd_text) TRY(L.bwd_text(m, m->s2));
    HIP_TRY(hipEventRecord(m->ev_join_b, m->s2));
    TRY(vision_backward(m, B, m->cp_unscale, s));
    HIP_TRY(hipStreamWaitEvent(s, m->ev_join_b, 0));
    return L.bwd ? L.bwd(m, s) : MUDPT_OK;
}

// ---- class-parallel phases (SURVEY 8e second axis; the reference runs all C prompts on every replica, trainers/mudpt.py:142-156,230-233) ----
// A handle with mudpt_set_class_shard(c0, c1) encodes classes [c0, c1) only.  One step on every rank:
//   mudpt_cp_forward          both towers; this rank's rows of the [n_cls, e] text-feature table, the other rows zero
//   <exchange 1>              all-reduce(sum) (or all-gather) of the table  (mudpt_cp_buffers: feat)
//   mudpt_cp_head             logits, loss and the head's backward over the LOCAL images and ALL classes -> dimg, dfeat [n_cls, e]
//   <exchange 2>              all-reduce(sum) of dfeat: every rank's images contribute to every class
//   mudpt_cp_backward         VISION part may be enqueued before exchange 2 completes; TEXT part (local classes + prompt learner) after it
//   <the usual all-reduce of the gradient bucket>   text-side gradients are partial sums over classes, vision-side ones over images
extern "C" int mudpt_set_class_shard(mudpt_model* m, int32_t c0, int32_t c1) {
    ARG_CHECK(m, "set_class_shard: null model");
    NOT_FROZEN(m, "set_class_shard");
    if (m->cocoop) { set_error("set_class_shard: CoCoOp's text features depend on the image; shard the batch instead"); return MUDPT_ERR_ARG; }
    if (m->coop) { set_error("set_class_shard: class-parallel CoOp is not implemented; shard the batch instead"); return MUDPT_ERR_ARG; }
    if (m->indep) { set_error("set_class_shard: class-parallel VPT / MPT is not implemented; shard the batch instead"); return MUDPT_ERR_ARG; }
    if (m->umudpt) { set_error("set_class_shard: class-parallel UMuDPT is not implemented; shard the batch instead"); return MUDPT_ERR_ARG; }
    ARG_CHECK(c0 >= 0 && c1 > c0 && c1 <= m->cfg.n_cls, "set_class_shard: [%d, %d) is not a non-empty range of the %d classes", c0, c1, m->cfg.n_cls);
    m->c0 = c0; m->ct = c1 - c0;
    m->sharded = !(c0 == 0 && c1 == m->cfg.n_cls);
    m->prompts_set = false;  // the text tower is sized and its tables are built by the next mudpt_set_class_prompts
    m->text_valid = false;
    m->cp_stage = 0;
    return MUDPT_OK;
}
// the class-parallel phases' refusal of every variant but MuDPT (CoCoOp: the phases' own argument checks)
static int cp_mudpt_only(const mudpt_model* m, const char* what) {
    NOT_FROZEN(m, what);
    ARG_CHECK(!(m && (m->coop || m->indep || m->umudpt)), "%s: not a MuDPT model (the class-parallel phases run MuDPT only)", what);
    return MUDPT_OK;
}
extern "C" int mudpt_cp_buffers(mudpt_model* m, float** feat, float** dfeat, size_t* numel) {
    TRY(cp_mudpt_only(m, "cp_buffers"));
    ARG_CHECK(m && !m->cocoop, "cp_buffers: not a MuDPT model");
    if (feat) *feat = m->txt_f;
    if (dfeat) *dfeat = m->dtxt;
    if (numel) *numel = (size_t)m->cfg.n_cls * m->cfg.embed_dim;
    return MUDPT_OK;
}
extern "C" int mudpt_cp_forward(mudpt_model* m, const float* images, int32_t B, int32_t flags, void* stream) {
    TRY(cp_mudpt_only(m, "cp_forward"));
    TRY(ready(m, B, false));
    ARG_CHECK(images && !m->cocoop, "cp_forward: null images / not a MuDPT model");
    const bool reuse = (flags & MUDPT_FWD_REUSE_TEXT) != 0;
    if (reuse && !m->text_valid) { set_error("cp_forward: MUDPT_FWD_REUSE_TEXT before any text-tower pass"); return MUDPT_ERR_STATE; }
    m->train_fwd = (flags & MUDPT_FWD_TRAINING) != 0;
    TRY(towers_forward(m, images, B, (hipStream_t)stream, reuse));
    m->cp_B = B; m->cp_stage = 1;
    return MUDPT_OK;
}
extern "C" int mudpt_cp_head(mudpt_model* m, const int64_t* labels, int32_t B, float grad_scale, float* loss, float* logits, int32_t flags, void* stream) {
    TRY(cp_mudpt_only(m, "cp_head"));
    TRY(ready(m, B, labels != nullptr));
    ARG_CHECK(!m->cocoop && (labels ? loss != nullptr : logits != nullptr), "cp_head: training needs labels and loss, inference needs logits");
    if (m->cp_stage < 1 || m->cp_B != B) { set_error("cp_head: call mudpt_cp_forward with the same batch first"); return MUDPT_ERR_STATE; }
    hipStream_t s = (hipStream_t)stream;
    if (!labels) {  // inference: logits only (flags & MUDPT_FWD_REUSE_TEXT: the normalised table of the previous call)
        TRY(head_forward(m, B, (flags & MUDPT_FWD_REUSE_TEXT) != 0, s));
        HIP_TRY(hipMemcpyAsync(logits, m->logits, (size_t)B * m->cfg.n_cls * 4, hipMemcpyDeviceToDevice, s));
        m->cp_stage = 0;
        return MUDPT_OK;
    }
    HIP_TRY(hipMemsetAsync(m->grads, 0, m->total * 4, s));
    TRY(head_train(m, labels, B, grad_scale, loss, logits, s));
    m->cp_stage = 2;
    return MUDPT_OK;
}
extern "C" int mudpt_cp_backward(mudpt_model* m, int32_t part, void* stream) {
    TRY(cp_mudpt_only(m, "cp_backward"));
    ARG_CHECK(m && !m->cocoop && (part == MUDPT_CP_VISION || part == MUDPT_CP_TEXT), "cp_backward: part must be MUDPT_CP_VISION or MUDPT_CP_TEXT");
    hipStream_t s = (hipStream_t)stream;
    if (part == MUDPT_CP_VISION) {
        if (m->cp_stage != 2) { set_error("cp_backward: call mudpt_cp_head (training) first"); return MUDPT_ERR_STATE; }
        TRY(vision_backward(m, m->cp_B, m->cp_unscale, s));
        m->cp_stage = 3;
        return MUDPT_OK;
    }
    if (m->cp_stage != 3) { set_error("cp_backward: the vision part comes first"); return MUDPT_ERR_STATE; }
    TRY(text_backward(m, m->cp_unscale, s));  // on the caller's stream: ordered behind its exchange of dfeat
    m->cp_stage = 0;
    return prompt_learner_backward(m, s);
}

extern "C" int mudpt_sgd_step(mudpt_model* m, float lr, float momentum, float wd, float dampening, int32_t nesterov, void* stream) {
    NOT_FROZEN(m, "sgd_step");
    ARG_CHECK(m && m->params && m->grads, "sgd_step: parameters / gradients not bound");
    TRY(launch_sgd(m->params, m->grads, m->momentum, m->total, lr, momentum, wd, dampening, nesterov != 0, m->sgd_first, (hipStream_t)stream));
    m->sgd_first = false;
    return MUDPT_OK;
}
extern "C" int mudpt_sgd_reset(mudpt_model* m) {
    ARG_CHECK(m, "sgd_reset: null model");
    m->sgd_first = true;
    return MUDPT_OK;
}

// mudpt_optim -> the launcher's arguments; the buffers are the caller's
static OptimArgs optim_args(const mudpt_optim& o, float* p, const float* g, int64_t n) {
    OptimArgs a;
    a.algo = o.algo; a.lr = o.lr; a.beta1 = o.beta1; a.beta2 = o.beta2; a.eps = o.eps; a.weight_decay = o.weight_decay; a.momentum = o.momentum;
    a.alpha = o.alpha; a.dampening = o.dampening; a.nesterov = o.nesterov != 0; a.amsgrad = o.amsgrad != 0; a.centered = o.centered != 0; a.step = o.step;
    a.p = p; a.g = g; a.n = n;
    for (int k = 0; k < 3; ++k) a.state[k] = o.state[k];
    return a;
}
extern "C" int mudpt_optim_step(mudpt_model* m, const mudpt_optim* optim, void* stream) {
    NOT_FROZEN(m, "optim_step");
    ARG_CHECK(m && optim, "optim_step: null argument");
    ARG_CHECK(m->params && m->grads, "optim_step: parameters / gradients not bound");
    return launch_optim(optim_args(*optim, m->params, m->grads, (int64_t)m->total), (hipStream_t)stream);
}

// ---- data-parallel exchange for hosts without torch.distributed ---------------------------------------------------------------
// The ONE collective of a step: sum of the flat gradient bucket over the ranks of an RCCL communicator the caller
// created (ncclCommInitRank; one process per GPU).  RCCL is resolved at first use from the process (librccl.so.1, the SONAME torch
// ships and /opt/rocm installs), so the library has no link-time dependency on it and single-GPU hosts never load it.
typedef int (*nccl_allreduce_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
static nccl_allreduce_fn resolve_allreduce() {
    static nccl_allreduce_fn fn = nullptr;
    if (fn) return fn;
    void* sym = dlsym(RTLD_DEFAULT, "ncclAllReduce");
    if (!sym) {
        for (const char* name : {"librccl.so.1", "librccl.so"}) {
            if (void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL)) {  // returns the already-loaded copy when the process has one
                sym = dlsym(h, "ncclAllReduce");
                if (sym) break;
            }
        }
    }
    fn = (nccl_allreduce_fn)sym;
    return fn;
}
extern "C" int mudpt_allreduce_grads(mudpt_model* m, void* nccl_comm, void* stream) {
    NOT_FROZEN(m, "allreduce_grads");
    ARG_CHECK(m && nccl_comm, "allreduce_grads: null model / communicator");
    if (!m->grads) { set_error("allreduce_grads: no gradient bucket bound"); return MUDPT_ERR_STATE; }
    nccl_allreduce_fn fn = resolve_allreduce();
    if (!fn) { set_error("allreduce_grads: RCCL (librccl.so.1) is not loadable in this process: %s", dlerror()); return MUDPT_ERR_STATE; }
    const int rc = fn(m->grads, m->grads, m->total, /*ncclFloat32*/ 7, /*ncclSum*/ 0, nccl_comm, (hipStream_t)stream);
    if (rc != 0) { set_error("allreduce_grads: ncclAllReduce failed with ncclResult_t %d", rc); return MUDPT_ERR_HIP; }
    return MUDPT_OK;
}

extern "C" int mudpt_set_loss_scale(mudpt_model* m, float loss_scale) {
    ARG_CHECK(m && loss_scale > 0.f && std::isfinite(loss_scale), "set_loss_scale: scale must be positive and finite");
    m->loss_scale = loss_scale;
    return MUDPT_OK;
}

// Per-handle tuning knobs for A/B runs in one process (tools/gemm_bench.py, tests); state of THIS model only.
extern "C" int mudpt_model_set(mudpt_model* m, const char* name, int32_t value) {
    ARG_CHECK(m && name, "model_set: null argument");
    if (!strcmp(name, "gemm_variant")) { m->gemm_variant = value; return MUDPT_OK; }
    // both stream copies are always allocated.  lp_grad = 0 (bf16 mode) also returns the forward's update stream to fp32, as before the two were separate knobs
    if (!strcmp(name, "lp_grad")) { m->lp_grad = value != 0; if (m->dtype == MUDPT_BF16) m->lp_upd = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "lp_upd")) { m->lp_upd = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "gelu_q8")) { m->gelu_q8 = value != 0; return MUDPT_OK; }  // between steps only: the backward decodes what the forward stored
    if (!strcmp(name, "txt_trim")) { m->txt_trim = value != 0; m->prompts_set = false; return MUDPT_OK; }  // read by the next mudpt_set_class_prompts
    if (!strcmp(name, "attn_two_kernels")) { m->attn_two_kernels = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "fwd_split_k")) { m->fwd_split_k = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "attn_fused_w1")) { m->attn_fused_w1 = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "split_k")) { m->split_k = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "attn_window")) { m->attn_window = value != 0; return MUDPT_OK; }
    if (!strcmp(name, "last_single")) { m->last_single = value != 0; return MUDPT_OK; }  // (a tower with the fp32 attention forward runs the general kernels anyway)
    if (!strcmp(name, "txt_bucket_cost")) { m->txt_bucket_cost = value > 0 ? value : 0; m->prompts_set = false; return MUDPT_OK; }
    if (!strcmp(name, "txt_buckets")) { m->txt_buckets = value > 1 ? value : 1; m->prompts_set = false; return MUDPT_OK; }  // read by the next mudpt_set_class_prompts
    if (!strcmp(name, "prof_stride")) { m->prof_stride = value > 1 ? value : 1; return MUDPT_OK; }
    if (!strcmp(name, "cocoop_chunk")) { m->cocoop_chunk = value; m->prompts_set = false; return MUDPT_OK; }  // likewise
    // Split operands (Tower::split).  Effective from the next forward: the low-half buffers and the e4m3 weights exist whenever
    // the tower may split at all (vision tower: the parity mode MUDPT_F32; text tower: MUDPT_F16 and MUDPT_F32).
    //   vis_lo / txt_lo          0 = no low halves, 1 = fp16 pairs (22 bits), 2 = e4m3 remainders on the fp8 matrix pipe (vision tower only)
    //   txt_split                the round-2 name of txt_lo = 0 / 1
    //   vis_sites / txt_sites    bit mask of the sites that take part (model.cpp Site: 1 in_proj, 2 out_proj, 4 c_fc, 8 c_proj, 16 patch embed)
    //   vis_exact_attn / txt_exact_attn   attention forward in fp32 (attention_exact.hip); parity mode only
    for (Tower* t : {&m->vis, &m->txt}) {
        const char* pre = t == &m->vis ? "vis_" : "txt_";
        if (strncmp(name, pre, 4)) continue;
        const char* k = name + 4;
        if (!strcmp(k, "lo") || (t == &m->txt && !strcmp(k, "split"))) {
            if (value != LO_NONE && !t->may_split) { set_error("model_set: %s needs a mode whose %s tower keeps low halves (dtype fp32%s)", name, t == &m->vis ? "vision" : "text", t == &m->txt ? " or fp16" : ""); return MUDPT_ERR_STATE; }
            ARG_CHECK(value == LO_NONE || value == LO_F16 || (value == LO_F8 && !t->w.empty() && t->w[0].w_in8), "model_set: %s = %d is not available for this tower", name, value);
            t->split = value;
            m->text_valid = false;
            return MUDPT_OK;
        }
        if (!strcmp(k, "sites")) { t->sites = value & 0x1f; m->text_valid = false; return MUDPT_OK; }
        if (!strcmp(k, "exact_attn")) {
            if (value && !(t->may_split && m->exact)) { set_error("model_set: %s needs the parity mode (dtype fp32)", name); return MUDPT_ERR_STATE; }
            t->exact_attn = value != 0;
            m->text_valid = false;
            return MUDPT_OK;
        }
    }
    set_error("model_set: unknown knob '%s'", name);
    return MUDPT_ERR_ARG;
}

extern "C" int mudpt_profile_enable(mudpt_model* m, int32_t enable) {
    ARG_CHECK(m, "profile_enable: null model");
    m->prof = enable != 0;
    m->prof_mask = enable == 1 ? 1 : enable;  // 1 = the dominant kernel only (class 0); otherwise a bit mask of MUDPT_PROF_CLASSES classes
    m->ev_used = 0;
    m->ev_rec.clear();
    m->exec_flop = 0;
    m->pp_seen = 0;
    return MUDPT_OK;
}
// Synchronises the device; sums per kernel class over the launches recorded since the last enable / read, then clears the records.
// out arrays have MUDPT_PROF_CLASSES entries: ms, work (class 0: algorithmic FLOPs 2 M N K; classes 1-4: algorithmic HBM bytes), launches.
extern "C" int mudpt_profile_read_classes(mudpt_model* m, double* ms, double* work, int64_t* launches, double* executed_flop) {
    ARG_CHECK(m && ms && work && launches, "profile_read: null argument");
    HIP_TRY(hipDeviceSynchronize());
    for (int c = 0; c < PC_COUNT; ++c) { ms[c] = 0; work[c] = 0; launches[c] = 0; }
    for (size_t i = 0; i < m->ev_used; i += 2) {
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, m->ev[i], m->ev[i + 1]));
        const mudpt_model::ProfRec& r = m->ev_rec[i / 2];
        ms[r.cls] += t; work[r.cls] += r.work; launches[r.cls] += 1;
    }
    if (executed_flop) *executed_flop = m->exec_flop;
    m->ev_used = 0;
    m->ev_rec.clear();
    m->exec_flop = 0;
    return MUDPT_OK;
}
extern "C" int mudpt_profile_read(mudpt_model* m, double* gemm_ms, double* gemm_flop, int64_t* launches) {
    ARG_CHECK(m && gemm_ms && gemm_flop && launches, "profile_read: null argument");
    double ms[PC_COUNT], work[PC_COUNT];
    int64_t n[PC_COUNT];
    if (int rc = mudpt_profile_read_classes(m, ms, work, n, nullptr)) return rc;
    *gemm_ms = ms[PC_GEMM]; *gemm_flop = work[PC_GEMM]; *launches = n[PC_GEMM];
    return MUDPT_OK;
}

// Copy an internal fp32 activation of the LAST call to the host (synchronises the device): per-block parity tests.
// names: "vis.x_in.<i>", "vis.x_out", "txt.x_in.<i>", "txt.x_out", "image_features", "text_features"
extern "C" int mudpt_debug_read(mudpt_model* m, const char* name, int32_t batch, float* host_out, size_t capacity, size_t* numel) {
    ARG_CHECK(m && name && numel, "debug_read: null argument");
    const std::string k(name);
    const mudpt_config& c = m->cfg;
    const float* src = nullptr;
    size_t n = 0;
    auto tower = [&](Tower& t, const std::string& rest, int nseq) {
        if (t.packed() && rest != "x_out") return;  // packed in length buckets: no [seq, L, d] view (set txt_buckets = 1 to tap)
        n = (size_t)nseq * t.L * t.d;
        if (rest == "x_out") { src = t.xout_sel; n = (size_t)nseq * t.d; }  // the used row (CLS / EOT) of every sequence only
        else if (rest.rfind("x_in.", 0) == 0) {
            const int i = atoi(rest.c_str() + 5);
            if (i >= 0 && i < t.layers) src = t.a[i].x_in;
        }
    };
    ARG_CHECK(batch > 0 && batch <= c.max_batch, "debug_read: bad batch %d", batch);
    if (k.rfind("vis.", 0) == 0) tower(m->vis, k.substr(4), batch);
    else if (k.rfind("txt.", 0) == 0) tower(m->txt, k.substr(4), m->ct);  // this handle's classes
    else if (k == "image_features") { src = m->img_f; n = (size_t)batch * c.embed_dim; }
    else if (k == "text_features") { src = m->frozen ? m->txt_n : m->txt_f; n = (size_t)c.n_cls * c.embed_dim; }  // frozen: the ensembled, normalised table
    else if (m->umudpt && !m->uumudpt && (k == "umudpt.G" || k == "umudpt.dG")) { src = k == "umudpt.G" ? m->pg_G : m->pg_dG; n = (size_t)c.depth * c.n_ctx * c.v_width; }
    else if (m->uumudpt && (k == "uumudpt.G" || k == "uumudpt.dG")) { src = k == "uumudpt.G" ? m->pg_G : m->pg_dG; n = (size_t)c.depth * c.n_ctx * c.v_width; }
    else if (m->uumudpt && c.depth > 1 && (k == "uumudpt.T" || k == "uumudpt.dT")) { src = k == "uumudpt.T" ? m->pg2_T : m->d_txt_deep; n = (size_t)(c.depth - 1) * c.n_ctx * c.embed_dim; }
    else if (k == "text_launches" || (m->rn && k == "conv2d_launches")) {  // host counters, not device tensors
        *numel = 1;
        if (host_out) { ARG_CHECK(capacity >= 1, "debug_read: capacity 0"); host_out[0] = (float)(k == "text_launches" ? m->text_launches : m->rn->conv2d_launches); }
        return MUDPT_OK;
    }
    ARG_CHECK(src, "debug_read: unknown tensor '%s'", name);
    *numel = n;
    if (!host_out) return MUDPT_OK;
    ARG_CHECK(capacity >= n, "debug_read: capacity %zu < %zu", capacity, n);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_out, src, n * 4, hipMemcpyDeviceToHost));
    return MUDPT_OK;
}

// ---- single kernels ---------------------------------------------------------------------------------------------
extern "C" int mudpt_gemm(int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
                          const float* bias, void* out0, int32_t ldo0, void* out1, int32_t ldo1, const void* aux, int32_t ldaux, int32_t patches,
                          int32_t seq_len, const float* pos, int32_t variant, void* stream) {
    GemmOpts o;
    o.variant = variant & ~0x30000;
    if (variant & 0x10000) {  // unit-test hook: allow split K, with a per-device scratch made on first use (never freed)
        static float* scratch[64] = {};
        const int dev = current_device();
        if (!scratch[dev]) HIP_TRY(hipMalloc((void**)&scratch[dev], mudpt_model::kScratchElems * 4));
        o.scratch = scratch[dev];
        o.scratch_elems = mudpt_model::kScratchElems;
    }
    GemmArgs a; a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.bias = bias; a.out0 = out0; a.ldo0 = ldo0; a.out1 = out1; a.ldo1 = ldo1;
    a.aux = aux; a.ldaux = ldaux; a.patches = patches; a.seq_len = seq_len; a.pos = pos;
    a.gelu_q8 = (variant & 0x20000) != 0;  // unit-test hook: QuickGELU' in 8 bits (epilogues 1 / 3; ldo0 / ldaux are then BYTE strides)
    return launch_gemm(dtype, epi, a, (hipStream_t)stream, o);
}
// the decision launch_gemm takes for mudpt_gemm's / mudpt_gemm_split's arguments (bit 16 of variant: the scratch mudpt_gemm would pass)
extern "C" int mudpt_gemm_form(int32_t epi, int32_t M, int32_t N, int32_t K, int32_t ldo0, int32_t ldo1, int32_t ldaux, int32_t lo_mode, int32_t variant, int32_t ncu) {
    static float some_scratch = 0.f;  // never dereferenced: gemm_form only asks whether there is one
    GemmOpts o;
    o.variant = variant & ~0x30000;
    if (variant & 0x10000) { o.scratch = &some_scratch; o.scratch_elems = mudpt_model::kScratchElems; }
    GemmArgs a; a.M = M; a.N = N; a.K = K; a.ldo0 = ldo0; a.ldo1 = ldo1; a.ldaux = ldaux; a.lo_mode = lo_mode;
    if (ncu <= 0 || !gemm_shape_ok(epi, a)) return -1;
    const GemmPlan p = gemm_form(epi, a, o, ncu);
    return (int)p.form | p.slices << 8;
}
extern "C" int mudpt_gemm_split(int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K, const void* A, const void* A_lo, int32_t lo_mode, int32_t lda,
                                const void* B, const void* B8, int32_t b8_scale, int32_t ldb, const float* bias, void* out0, int32_t ldo0, void* out1,
                                void* out1_lo, int32_t out1_lo_mode, int32_t ldo1, const void* aux, int32_t ldaux, int32_t variant, void* stream) {
    GemmOpts o;
    o.variant = variant;
    GemmArgs a; a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.bias = bias; a.out0 = out0; a.ldo0 = ldo0; a.out1 = out1; a.ldo1 = ldo1;
    a.aux = aux; a.ldaux = ldaux; a.A_lo = A_lo; a.lo_mode = lo_mode; a.B8 = B8; a.b8_scale = b8_scale; a.out1_lo = out1_lo; a.out1_lo_mode = out1_lo ? out1_lo_mode : (int)LO_F16;
    return launch_gemm(dtype, epi, a, (hipStream_t)stream, o);
}
extern "C" int mudpt_optim_apply(const mudpt_optim* optim, float* p, const float* g, int64_t n, void* stream) {
    ARG_CHECK(optim, "optim_apply: null argument");
    return launch_optim(optim_args(*optim, p, g, n), (hipStream_t)stream);
}
extern "C" int mudpt_e4m3_from_f32(const float* in_host, uint8_t* out_host, size_t n, int32_t shift) {
    ARG_CHECK(in_host && out_host, "e4m3_from_f32: null argument");
    for (size_t i = 0; i < n; ++i) out_host[i] = f32_to_e4m3(std::ldexp(in_host[i], shift));
    return MUDPT_OK;
}
extern "C" int mudpt_layernorm_fwd_split(int32_t dtype, const float* x, int32_t ldx, const float* gamma, const float* beta, void* out, void* out_lo, int32_t lo_mode,
                                         int32_t ldo, int32_t rows, int32_t d, void* stream) {
    LnFwdArgs a; a.x = x; a.ldx = ldx; a.gamma = gamma; a.beta = beta; a.out = out; a.out_lo = out_lo; a.lo_mode = lo_mode; a.ldo = ldo; a.rows = rows; a.d = d;
    ARG_CHECK(out_lo && (lo_mode == LO_F16 || lo_mode == LO_F8), "layernorm_fwd_split: needs out_lo and lo_mode 1 / 2");
    return launch_ln_fwd(dtype, a, (hipStream_t)stream);
}
extern "C" int mudpt_layernorm_fwd(int32_t dtype, const float* x, int32_t ldx, const int32_t* row_index, const float* gamma, const float* beta, void* out,
                                   int32_t ldo, int32_t out_f32, float* mean, float* rstd, int32_t rows, int32_t d, void* stream) {
    LnFwdArgs a; a.x = x; a.ldx = ldx; a.row_index = row_index; a.gamma = gamma; a.beta = beta; a.out = out; a.ldo = ldo; a.out_f32 = out_f32 != 0;
    a.mean = mean; a.rstd = rstd; a.rows = rows; a.d = d;
    return launch_ln_fwd(dtype, a, (hipStream_t)stream);
}
extern "C" int mudpt_layernorm_bwd(int32_t dtype, const void* dy, int32_t lddy, int32_t dy_f32, const float* x, int32_t ldx, const int32_t* row_index,
                                   const float* mean, const float* rstd, const float* gamma, const float* dres, int32_t lddres, float* dx, int32_t lddx,
                                   void* dx_lp, int32_t lddx_lp, int32_t rows, int32_t d, void* stream) {
    LnBwdArgs a; a.dy = dy; a.lddy = lddy; a.dy_f32 = dy_f32 != 0; a.x = x; a.ldx = ldx; a.row_index = row_index; a.mean = mean; a.rstd = rstd; a.gamma = gamma;
    a.dres = dres; a.lddres = lddres; a.dx = dx; a.lddx = lddx; a.dx_lp = dx_lp; a.lddx_lp = lddx_lp; a.rows = rows; a.d = d;
    return launch_ln_bwd(dtype, a, (hipStream_t)stream);
}
extern "C" int mudpt_layernorm_fwd_fused(int32_t dtype, const float* x, int32_t ldx, const float* add, const void* add_lp, int32_t ldadd, const float* ov_rows,
                                         int32_t ov_row0, int32_t ov_n, int32_t ov_L, float* xout, int32_t ldxout, const float* gamma, const float* beta, void* out,
                                         int32_t ldo, int32_t out_f32, float* mean, float* rstd, int32_t rows, int32_t d, void* stream) {
    LnFwdArgs a; a.x = x; a.ldx = ldx; a.add = add; a.add_lp = add_lp; a.ldadd = ldadd; a.xout = xout; a.ldxout = ldxout; a.gamma = gamma; a.beta = beta;
    a.out = out; a.ldo = ldo; a.out_f32 = out_f32 != 0; a.mean = mean; a.rstd = rstd; a.rows = rows; a.d = d;
    if (ov_rows) { a.ov_rows = ov_rows; a.ov_row0 = ov_row0; a.ov_n = ov_n; a.ov_L = ov_L; }
    return launch_ln_fwd(dtype, a, (hipStream_t)stream);
}
extern "C" int mudpt_head(const float* img, const float* txt, const int64_t* labels, float scale, float grad_scale, int32_t B, int32_t C, int32_t e,
                          float* logits, float* loss, float* dimg, float* dtxt, void* stream) {
    ARG_CHECK(img && txt && logits && B > 0 && C > 0 && e > 0, "head: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    float* scratch = nullptr;
    const size_t need = (size_t)B * e + (size_t)C * e + B + C + (size_t)B * C + B;
    HIP_TRY(hipMalloc((void**)&scratch, need * 4));
    HeadArgs h; h.img = img; h.txt = txt; h.labels = labels; h.scale = scale; h.logits = logits; h.loss = loss; h.dimg = dimg; h.dtxt = dtxt;
    h.img_n = scratch; h.txt_n = h.img_n + (size_t)B * e; h.img_inv = h.txt_n + (size_t)C * e; h.txt_inv = h.img_inv + B;
    h.dlogits = h.txt_inv + C; h.row_loss = h.dlogits + (size_t)B * C; h.grad_scale = grad_scale; h.B = B; h.C = C; h.e = e;
    int rc;
    if (head_fused_fits(h, labels != nullptr)) rc = labels ? launch_head_fused_train(h, s) : launch_head_fused_fwd(h, s);
    else {
        rc = launch_head_fwd(h, s);
        if (!rc && labels) rc = launch_head_bwd(h, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(scratch);
    return rc;
}
extern "C" int mudpt_reduce_rows(int32_t dtype, float* src, void* src_lp, int32_t B, int32_t L, int32_t d, int32_t row0, int32_t n, float* out,
                                 int32_t zero_src, int32_t accumulate, float scale, void* stream) {
    return launch_reduce_rows(dtype, src, src_lp, B, L, d, row0, n, out, zero_src != 0, accumulate != 0, scale, (hipStream_t)stream);
}
extern "C" int mudpt_cocoop_dbias(int32_t dtype, const float* dx_f32, const void* dx_lp, float* dbias, int32_t B, int32_t C, int32_t L, int32_t d, int32_t n,
                                  float scale, void* stream) {
    return launch_cocoop_dbias(dtype, dx_f32, dx_lp, dbias, B, C, L, d, n, scale, (hipStream_t)stream);
}
extern "C" int mudpt_coop_dctx(int32_t dtype, const float* dx_f32, const void* dx_lp, const int32_t* rows, float* dctx, int32_t C, int32_t n, int32_t d,
                               int32_t csc, float scale, void* stream) {
    return launch_coop_dctx(dtype, dx_f32, dx_lp, rows, dctx, C, n, d, csc != 0, scale, (hipStream_t)stream);
}
extern "C" int mudpt_sgemm(int32_t tA, int32_t tB, int32_t M, int32_t N, int32_t K, float alpha, const float* A, int32_t lda, const float* B, int32_t ldb,
                           float beta, float* C, int32_t ldc, const float* bias, void* stream) {
    return launch_sgemm(tA != 0, tB != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, bias, (hipStream_t)stream);
}
extern "C" int mudpt_attention_fwd_single(int32_t dtype, const void* qkv, const void* q_sel, const int32_t* sel_rows, void* out_sel, float* lse_sel, int32_t B, int32_t L,
                                          int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv = qkv; a.sel_rows = sel_rows; a.B = B; a.L = L; a.H = H; a.causal = causal != 0;
    return launch_attn_fwd_single(dtype, a, q_sel, out_sel, nullptr, H * 64, lse_sel, (hipStream_t)stream);
}
extern "C" int mudpt_attention_bwd_single(int32_t dtype, const void* qkv, const void* q_sel, const int32_t* sel_rows, const void* out_sel, const void* dout_sel,
                                          const float* lse_sel, void* dqkv, void* dq_sel, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv = qkv; a.sel_rows = sel_rows; a.dqkv = dqkv; a.B = B; a.L = L; a.H = H; a.causal = causal != 0;
    return launch_attn_bwd_single(dtype, a, q_sel, out_sel, H * 64, dout_sel, lse_sel, dq_sel, (hipStream_t)stream);
}
extern "C" int mudpt_attention_padded_len(int32_t L) { return attn_padded_len(L); }
// The `causal` argument of mudpt_attention_fwd / _fwd_split / _bwd / _bwd_sel and the `flags` of mudpt_attention_form (bit meanings: include/mudpt.h at
// mudpt_attention_bwd): the mask and the window go into a, the kernel-choice switches are returned.
static AttnOpts attn_flags(int32_t flags, bool bwd, AttnArgs& a) {
    AttnOpts o;
    a.causal = (flags & 1) != 0;
    if (!bwd) {
        o.tiled_fwd_16 = (flags & 2) != 0;
        return o;
    }
    o.two_kernels = (flags & 2) != 0; o.fused_w1 = (flags & 4) != 0; o.force_fused = (flags & 12) != 0; o.sweep = (flags & 16) != 0;
    a.win_row0 = (flags >> 8) & 0xfff; a.win_n = (flags >> 20) & 0xff;
    return o;
}
extern "C" int mudpt_attention_form(int32_t bwd, int32_t L, int32_t flags, int32_t sel) {
    if (L < 1 || L > 4096) return -1;
    static const int one_row = 0;
    AttnArgs a; a.L = L; a.sel_rows = bwd && sel ? &one_row : nullptr;
    const AttnOpts o = attn_flags(sel ? flags & 1 : flags, bwd != 0, a);  // mudpt_attention_bwd_sel reads bit 0 only
    return attn_form(a, o, bwd != 0);
}
extern "C" int mudpt_attention_fwd(int32_t dtype, const void* qkv, void* out, float* lse, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv = qkv; a.out = out; a.lse = lse; a.B = B; a.L = L; a.H = H;
    const AttnOpts o = attn_flags(causal, false, a);
    return launch_attn_fwd(dtype, a, (hipStream_t)stream, o);
}
extern "C" int mudpt_attention_fwd_exact(const float* qkv32, void* qkv_lp, void* out_hi, void* out_lo, int32_t lo_mode, int32_t ld_out, float* lse, int32_t B, int32_t L,
                                         int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv32 = qkv32; a.qkv_lp = qkv_lp; a.out = out_hi; a.out_lo = out_lo; a.lo_mode = out_lo ? lo_mode : (int)LO_F16; a.ld_out = ld_out; a.lse = lse; a.B = B; a.L = L; a.H = H; a.causal = causal != 0;
    return launch_attn_fwd_exact(a, (hipStream_t)stream);
}
extern "C" int mudpt_attention_bwd(int32_t dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv, int32_t B,
                                   int32_t L, int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv = qkv; a.out = (void*)out; a.dout = dout; a.lse = (float*)lse; a.delta = delta; a.dqkv = dqkv; a.B = B; a.L = L; a.H = H;
    const AttnOpts o = attn_flags(causal, true, a);
    return launch_attn_bwd(dtype, a, (hipStream_t)stream, o);
}
// ---- the launchers' production forms, one thin argument-packing export each (tests/test_kernels_gpu.py, tests/test_movers_gpu.py) ----
extern "C" int mudpt_gemm_split_patch(int32_t dtype, int32_t epi, int32_t M, int32_t N, int32_t K, const void* A, const void* A_lo, int32_t lo_mode, int32_t lda,
                                      const void* B, const void* B8, int32_t b8_scale, int32_t ldb, const float* bias, void* out0, int32_t ldo0, void* out1,
                                      void* out1_lo, int32_t out1_lo_mode, int32_t ldo1, const void* aux, int32_t ldaux, int32_t patches, int32_t seq_len,
                                      const float* pos, int32_t variant, void* stream) {
    GemmOpts o;
    o.variant = variant;
    GemmArgs a; a.A = A; a.B = B; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldb = ldb; a.bias = bias; a.out0 = out0; a.ldo0 = ldo0; a.out1 = out1; a.ldo1 = ldo1;
    a.aux = aux; a.ldaux = ldaux; a.A_lo = A_lo; a.lo_mode = lo_mode; a.B8 = B8; a.b8_scale = b8_scale; a.out1_lo = out1_lo; a.out1_lo_mode = out1_lo ? out1_lo_mode : (int)LO_F16;
    a.patches = patches; a.seq_len = seq_len; a.pos = pos;
    return launch_gemm(dtype, epi, a, (hipStream_t)stream, o);
}
extern "C" int mudpt_layernorm_bwd_ex(int32_t dtype, const void* dy, int32_t lddy, int32_t dy_f32, const float* x, int32_t ldx, const int32_t* row_index,
                                      const float* mean, const float* rstd, const float* gamma, const float* dres, const void* dres_lp, int32_t lddres,
                                      float* dx, int32_t lddx, void* dx_lp, int32_t lddx_lp, float* side, int32_t side_row0, int32_t side_n, int32_t side_L,
                                      size_t side_ldb, int32_t index_mode, int32_t rows, int32_t d, void* stream) {
    ARG_CHECK(index_mode >= 0 && index_mode <= 2, "layernorm_bwd_ex: index_mode must be 0 (compact), 1 (by_token) or 2 (stats_by_token)");
    LnBwdArgs a; a.dy = dy; a.lddy = lddy; a.dy_f32 = dy_f32 != 0; a.x = x; a.ldx = ldx; a.row_index = row_index; a.mean = mean; a.rstd = rstd; a.gamma = gamma;
    a.dres = dres; a.dres_lp = dres_lp; a.lddres = lddres; a.dx = dx; a.lddx = lddx; a.dx_lp = dx_lp; a.lddx_lp = lddx_lp; a.rows = rows; a.d = d;
    a.by_token = index_mode == 1; a.stats_by_token = index_mode == 2;
    if (side) { a.side = side; a.side_row0 = side_row0; a.side_n = side_n; a.side_L = side_L; a.side_ldb = side_ldb; }
    return launch_ln_bwd(dtype, a, (hipStream_t)stream);
}
extern "C" int mudpt_layernorm_fwd_ex(int32_t dtype, const float* x, int32_t ldx, const int32_t* row_index, const float* add, const void* add_lp, int32_t ldadd,
                                      const float* ov_rows, int32_t ov_row0, int32_t ov_n, int32_t ov_L, float* xout, int32_t ldxout, const float* gamma,
                                      const float* beta, void* out, void* out_lo, int32_t lo_mode, int32_t ldo, int32_t out_f32, float* mean, float* rstd,
                                      int32_t rows, int32_t d, void* stream) {
    LnFwdArgs a; a.x = x; a.ldx = ldx; a.row_index = row_index; a.add = add; a.add_lp = add_lp; a.ldadd = ldadd; a.xout = xout; a.ldxout = ldxout;
    a.gamma = gamma; a.beta = beta; a.out = out; a.out_lo = out_lo; a.lo_mode = lo_mode; a.ldo = ldo; a.out_f32 = out_f32 != 0; a.mean = mean; a.rstd = rstd;
    a.rows = rows; a.d = d;
    if (ov_rows) { a.ov_rows = ov_rows; a.ov_row0 = ov_row0; a.ov_n = ov_n; a.ov_L = ov_L; }
    return launch_ln_fwd(dtype, a, (hipStream_t)stream);
}
extern "C" int mudpt_attention_fwd_split(int32_t dtype, const void* qkv, void* out, void* out_lo, int32_t lo_mode, int32_t ld_out, float* lse, int32_t B, int32_t L,
                                         int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv = qkv; a.out = out; a.out_lo = out_lo; a.lo_mode = lo_mode; a.ld_out = ld_out; a.lse = lse; a.B = B; a.L = L; a.H = H;
    const AttnOpts o = attn_flags(causal, false, a);
    return launch_attn_fwd(dtype, a, (hipStream_t)stream, o);
}
extern "C" int mudpt_attention_fwd_single_split(int32_t dtype, const void* qkv, const void* q_sel, const int32_t* sel_rows, void* out_sel, void* out_lo,
                                                int32_t lo_mode, int32_t ld_out, float* lse_sel, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream) {
    AttnArgs a; a.qkv = qkv; a.sel_rows = sel_rows; a.lo_mode = lo_mode; a.B = B; a.L = L; a.H = H; a.causal = causal != 0;
    return launch_attn_fwd_single(dtype, a, q_sel, out_sel, out_lo, ld_out, lse_sel, (hipStream_t)stream);
}
extern "C" int mudpt_attention_bwd_sel(int32_t dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                                       const int32_t* sel_rows, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream) {
    ARG_CHECK(sel_rows, "attention_bwd_sel: null sel_rows");
    AttnArgs a; a.qkv = qkv; a.out = (void*)out; a.dout = dout; a.lse = (float*)lse; a.delta = delta; a.dqkv = dqkv; a.sel_rows = sel_rows; a.B = B; a.L = L; a.H = H;
    const AttnOpts o = attn_flags(causal & 1, true, a);  // bit 0 only: one wanted row leaves no kernel choice and takes no window
    return launch_attn_bwd(dtype, a, (hipStream_t)stream, o);
}
extern "C" int mudpt_head_ex(const float* img, const float* txt, const int64_t* labels, float scale, float grad_scale, int32_t B, int32_t B_total, int32_t C,
                             int32_t e, float* txt_n, float* txt_inv, float* logits, float* loss, float* row_loss, float* dimg, float* dtxt, int32_t path,
                             int32_t* path_taken, void* stream) {
    ARG_CHECK(img && txt_n && txt_inv && logits && B > 0 && B_total >= 0, "head_ex: bad arguments");  // C, e: the launchers' own checks
    ARG_CHECK(path == 0 || path == 1, "head_ex: path must be 0 (the dispatch of mudpt_head) or 1 (the unfused launchers)");
    ARG_CHECK(!labels || loss, "head_ex: training needs loss (dimg may be NULL: no image gradient)");
    hipStream_t s = (hipStream_t)stream;
    float* scratch = nullptr;
    const size_t need = (size_t)B * e + B + (size_t)B * C + B;
    HIP_TRY(hipMalloc((void**)&scratch, need * 4));
    HeadArgs h; h.img = img; h.txt = txt; h.labels = labels; h.scale = scale; h.logits = logits; h.loss = loss; h.dimg = dimg; h.dtxt = dtxt;
    h.img_n = scratch; h.img_inv = h.img_n + (size_t)B * e; h.dlogits = h.img_inv + B; h.row_loss = row_loss ? row_loss : h.dlogits + (size_t)B * C;
    h.txt_n = txt_n; h.txt_inv = txt_inv; h.grad_scale = grad_scale; h.B = B; h.B_total = B_total; h.C = C; h.e = e;
    const bool fused = path == 0 && head_fused_fits(h, labels != nullptr);
    if (path_taken) *path_taken = fused ? 0 : 1;
    int rc;
    if (fused) rc = labels ? launch_head_fused_train(h, s) : launch_head_fused_fwd(h, s);
    else {
        rc = launch_head_fwd(h, s);
        if (!rc && labels) rc = launch_head_bwd(h, s);
    }
    (void)hipStreamSynchronize(s);
    (void)hipFree(scratch);
    return rc;
}
extern "C" int mudpt_head_grad(const float* img_n, const float* img_inv, const float* txt_n, const float* txt_inv, const float* G, int64_t ldg, const float* Eimg,
                               const float* Etxt, float scale, float gmul, int32_t B, int32_t C, int32_t e, float* dimg, float* dtxt, int32_t path,
                               int32_t* path_taken, void* stream) {
    ARG_CHECK(path >= 0 && path <= 2, "head_grad: path must be 0 (the dispatch), 1 (the unfused launchers) or 2 (the fused kernels)");
    HeadGradArgs h; h.img_n = img_n; h.img_inv = img_inv; h.txt_n = txt_n; h.txt_inv = txt_inv; h.G = G; h.ldg = ldg; h.Eimg = Eimg; h.Etxt = Etxt;
    h.scale = scale; h.gmul = gmul; h.B = B; h.C = C; h.e = e; h.dimg = dimg; h.dtxt = dtxt;
    TRY(launch_head_grad(h, (hipStream_t)stream, path));
    if (path_taken) *path_taken = path == 2 || (path == 0 && head_grad_fused(h)) ? 0 : 1;  // a refused call writes nothing
    return MUDPT_OK;
}
extern "C" int mudpt_pair_head(const float* img, const float* txt, const int64_t* labels, float scale, float grad_scale, int32_t B, int32_t B_total, int32_t C,
                               int32_t e, float* logits, float* loss, float* row_loss, float* dtxt, void* stream) {
    ARG_CHECK(img && txt && logits && B > 0 && e > 0 && B_total >= 0, "pair_head: bad arguments");  // C: the launchers' own check
    ARG_CHECK(!labels || (loss && row_loss && dtxt), "pair_head: training needs loss, row_loss and dtxt");
    hipStream_t s = (hipStream_t)stream;
    float* scratch = nullptr;
    const size_t BC = (size_t)B * C, need = (size_t)B * e + B + BC * e + BC + BC;
    HIP_TRY(hipMalloc((void**)&scratch, need * 4));
    HeadArgs h; h.img = img; h.txt = txt; h.labels = labels; h.scale = scale; h.logits = logits; h.loss = loss; h.dtxt = dtxt; h.row_loss = row_loss;
    h.img_n = scratch; h.img_inv = h.img_n + (size_t)B * e; h.txt_n = h.img_inv + B; h.txt_inv = h.txt_n + BC * e; h.dlogits = h.txt_inv + BC;
    h.grad_scale = grad_scale; h.B = B; h.B_total = B_total > 0 ? B_total : B; h.C = C; h.e = e;  // as the CoCoOp step: the mean follows the chunks
    int rc = launch_l2norm(img, h.img_n, h.img_inv, B, e, s);
    if (!rc) rc = launch_pair_head_fwd(h, s);
    if (!rc && labels) rc = launch_pair_head_bwd(h, s);
    if (!rc && labels && B_total == 0) rc = launch_mean(row_loss, B, loss, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(scratch);
    return rc;
}
extern "C" int mudpt_patchify(int32_t dtype, const float* images, void* patches, void* patches_lo, int32_t lo_mode, int32_t B, int32_t image_size, int32_t patch,
                              int32_t ldk, void* stream) {
    if (patches_lo) return launch_patchify_split(dtype, images, patches, patches_lo, lo_mode, B, image_size, patch, ldk, (hipStream_t)stream);
    return launch_patchify(dtype, images, patches, B, image_size, patch, ldk, (hipStream_t)stream);
}
extern "C" int mudpt_set_rows(float* x, int32_t B, int32_t L, int32_t d, int32_t row0, int32_t n, const float* rows, const float* add, void* stream) {
    return launch_set_rows(x, B, L, d, row0, n, rows, add, (hipStream_t)stream);
}
extern "C" int mudpt_gather_rows(const void* src, size_t src_stride, const int32_t* rows, void* dst, size_t dst_stride, int32_t nrows, int32_t row_bytes, void* stream) {
    return launch_gather_rows(src, src_stride, rows, dst, dst_stride, nrows, row_bytes, (hipStream_t)stream);
}
extern "C" int mudpt_scatter_rows(const void* src, size_t src_stride, const int32_t* rows, void* dst, size_t dst_stride, int32_t nrows, int32_t row_bytes, void* stream) {
    return launch_scatter_rows(src, src_stride, rows, dst, dst_stride, nrows, row_bytes, (hipStream_t)stream);
}
extern "C" int mudpt_add_rows(int32_t dtype, const void* src, const int32_t* rows, void* dst, int32_t nrows, int32_t d, void* stream) {
    return launch_add_rows(dtype, src, rows, dst, nrows, d, (hipStream_t)stream);
}
extern "C" int mudpt_linear_bwd(int32_t R, int32_t out, int32_t in, const float* dy, const float* x, const float* W, float* dW, float* db, float* dx, void* stream) {
    return launch_linear_bwd(R, out, in, dy, x, W, dW, db, dx, (hipStream_t)stream);
}
extern "C" int mudpt_colsum(const float* A, int32_t M, int32_t N, int32_t lda, float* out, int32_t accumulate, void* stream) {
    return launch_colsum(A, M, N, lda, out, accumulate != 0, (hipStream_t)stream);
}
extern "C" int mudpt_add(const float* a, const float* b, float* y, size_t n, void* stream) { return launch_add(a, b, y, n, (hipStream_t)stream); }
extern "C" int mudpt_cast(int32_t dtype, const float* x, void* y, size_t n, void* stream) { return launch_cast(dtype, x, y, n, (hipStream_t)stream); }
extern "C" int mudpt_relu(float* y, size_t n, void* stream) { return launch_relu(y, n, (hipStream_t)stream); }
extern "C" int mudpt_relu_bwd(float* dy, const float* y, size_t n, void* stream) { return launch_relu_bwd(dy, y, n, (hipStream_t)stream); }
extern "C" int mudpt_cocoop_prompts(float* x0, const float* emb_pos, const float* ctx, const float* bias, const float* pos, int32_t B, int32_t C, int32_t L,
                                    int32_t d, int32_t n, void* stream) {
    return launch_cocoop_prompts(x0, emb_pos, ctx, bias, pos, B, C, L, d, n, (hipStream_t)stream);
}
extern "C" int mudpt_coop_splice(float* x, const float* ctx, const float* tpos, const int32_t* rows, const int32_t* pos, int32_t C, int32_t n, int32_t d,
                                 int32_t csc, void* stream) {
    return launch_coop_splice(x, ctx, tpos, rows, pos, C, n, d, csc != 0, (hipStream_t)stream);
}
// zero-shot CLIP's kernels (zeroshot.hip)
extern "C" int mudpt_embed_tokens(const float* table, int32_t vocab, const int32_t* tokens_dev, const int32_t* positions_dev, const float* pos, float* out,
                                  int32_t rows, int32_t d, void* stream) {
    return launch_embed_tokens(table, vocab, tokens_dev, positions_dev, pos, out, rows, d, (hipStream_t)stream);
}
extern "C" int mudpt_feature_ensemble(const float* f, float* acc, float* out, int32_t C, int32_t e, int32_t first, int32_t last, int32_t n_templates, void* stream) {
    return launch_feature_ensemble(f, acc, out, C, e, first != 0, last != 0, n_templates, (hipStream_t)stream);
}
// the linear probe's kernels (probe.hip)
extern "C" int mudpt_probe_gemm_nt(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb, const float* bias, float* C, int32_t ldc,
                                   void* stream) {
    return launch_probe_gemm_nt(M, N, K, A, lda, B, ldb, bias, C, ldc, (hipStream_t)stream);
}
extern "C" int mudpt_probe_gemm_tn(int32_t M, int32_t N, int32_t Kd, const float* A, int32_t lda, const float* B, int32_t ldb, float beta, const float* W, int32_t ldw,
                                   float* C, int32_t ldc, float* db, float* scratch, size_t scratch_numel, int32_t slices, void* stream) {
    return launch_probe_gemm_tn(M, N, Kd, A, lda, B, ldb, beta, W, ldw, C, ldc, db, scratch, scratch_numel, slices, (hipStream_t)stream);
}
extern "C" int mudpt_probe_gemm_tn_slices(int32_t M, int32_t N, int32_t Kd, int32_t slices, int32_t ncu) { return probe_tn_slices(M, N, Kd, slices, ncu); }
extern "C" int mudpt_probe_rows(float* Z, int32_t ldz, const int32_t* labels, int32_t rows, int32_t n_cls, float* row_loss, double* loss_sum, void* stream) {
    return launch_probe_rows(Z, ldz, labels, rows, n_cls, row_loss, loss_sum, (hipStream_t)stream);
}
extern "C" int mudpt_probe_argmax(const float* Z, int32_t ldz, int32_t rows, int32_t n_cls, int32_t* pred, const int32_t* labels, int32_t* count, void* stream) {
    return launch_probe_argmax(Z, ldz, rows, n_cls, pred, labels, count, (hipStream_t)stream);
}
// the test pass's evaluator (evaluate.hip): stateless, no model handle
extern "C" size_t mudpt_eval_state_numel(int32_t n_cls, int32_t with_cmat) { return eval_state_numel(n_cls, with_cmat); }
extern "C" int mudpt_eval_reset(int32_t* state, int32_t n_cls, int32_t with_cmat, void* stream) { return launch_eval_reset(state, n_cls, with_cmat, (hipStream_t)stream); }
extern "C" int mudpt_eval_accumulate(const float* logits, int32_t ldz, const int64_t* labels, int32_t rows, int32_t n_cls, int32_t* state, int32_t with_cmat,
                                     int32_t* pred, void* stream) {
    return launch_eval_accumulate(logits, ldz, labels, rows, n_cls, state, with_cmat, pred, (hipStream_t)stream);
}
extern "C" int mudpt_eval_finalize(const int32_t* state, int32_t n_cls, double* results, void* stream) {
    return launch_eval_finalize(state, n_cls, results, (hipStream_t)stream);
}
// top-k in the evaluator's order (topk.hip): stateless, no model handle
extern "C" int mudpt_topk(const float* logits, int32_t ldz, int32_t rows, int32_t n_cls, int32_t k, int32_t* index, float* value, float* prob, void* stream) {
    return launch_topk(logits, ldz, rows, n_cls, k, index, value, prob, (hipStream_t)stream);
}
extern "C" int mudpt_rank_accumulate(const float* logits, int32_t ldz, const int64_t* labels, int32_t rows, int32_t n_cls, int32_t kmax, int32_t* state,
                                     int32_t* rank, void* stream) {
    return launch_rank_accumulate(logits, ldz, labels, rows, n_cls, kmax, state, rank, (hipStream_t)stream);
}
// UMuDPT's prompt generator (promptgen.hip): its three kernels, and the whole block as the model path runs it
extern "C" int mudpt_layernorm_bwd_affine(const float* x, int32_t ldx, const float* mean, const float* rstd, const float* gamma, const float* dy, int32_t lddy,
                                          const float* dres, int32_t lddres, float* dx, int32_t lddx, float* dgamma, float* dbeta, int32_t accumulate,
                                          int32_t rows, int32_t d, void* stream) {
    LnBwdAffineArgs a; a.x = x; a.ldx = ldx; a.mean = mean; a.rstd = rstd; a.gamma = gamma; a.dy = dy; a.lddy = lddy; a.dres = dres; a.lddres = lddres;
    a.dx = dx; a.lddx = lddx; a.dgamma = dgamma; a.dbeta = dbeta; a.accumulate = accumulate != 0; a.rows = rows; a.d = d;
    return launch_ln_bwd_affine(a, (hipStream_t)stream);
}
extern "C" int mudpt_pg_attention_fwd(const float* qkv, float* out, float* probs, int32_t N, int32_t L, int32_t H, int32_t d_model, void* stream) {
    return launch_pg_attn_fwd(qkv, out, probs, N, L, H, d_model, (hipStream_t)stream);
}
extern "C" int mudpt_pg_attention_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int32_t N, int32_t L, int32_t H, int32_t d_model,
                                      void* stream) {
    return launch_pg_attn_bwd(qkv, probs, dout, dqkv, N, L, H, d_model, (hipStream_t)stream);
}
extern "C" int mudpt_quickgelu_fwd(const float* u, float* y, size_t n, void* stream) { return launch_quickgelu_fwd(u, y, n, (hipStream_t)stream); }
extern "C" int mudpt_quickgelu_bwd(const float* dy, const float* u, float* du, size_t n, void* stream) { return launch_quickgelu_bwd(dy, u, du, n, (hipStream_t)stream); }
extern "C" size_t mudpt_promptgen_workspace(int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v) {
    size_t ws = 0;
    if (pg_check_shape("promptgen_workspace", depth, n_ctx, d_t, d_v)) return 0;
    (void)pg_carve(nullptr, depth, n_ctx, d_t, &ws);
    return ws;
}
extern "C" size_t mudpt_promptgen_param_numel(int32_t d_t, int32_t d_v) { return d_t > 0 && d_v > 0 ? pg_params(nullptr, d_t, d_v).total : 0; }
static int promptgen_workspace_ok(const char* what, int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v, const float* ws, size_t ws_numel) {
    if (int r = pg_check_shape(what, depth, n_ctx, d_t, d_v)) return r;
    ARG_CHECK(ws && ws_numel >= mudpt_promptgen_workspace(depth, n_ctx, d_t, d_v), "%s: workspace of %zu elements, needs %zu", what, ws_numel,
              mudpt_promptgen_workspace(depth, n_ctx, d_t, d_v));
    return MUDPT_OK;
}
extern "C" int mudpt_promptgen_forward(int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v, const float* params, const float* X, float* G, float* workspace,
                                       size_t workspace_numel, void* stream) {
    if (int r = promptgen_workspace_ok("promptgen_forward", depth, n_ctx, d_t, d_v, workspace, workspace_numel)) return r;
    return pg_forward(depth, n_ctx, d_t, d_v, pg_params(params, d_t, d_v), X, G, pg_carve(workspace, depth, n_ctx, d_t, nullptr), (hipStream_t)stream);
}
extern "C" int mudpt_promptgen_backward(int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v, const float* params, const float* X, const float* dG, float* dX,
                                        float* grads, float* workspace, size_t workspace_numel, void* stream) {
    if (int r = promptgen_workspace_ok("promptgen_backward", depth, n_ctx, d_t, d_v, workspace, workspace_numel)) return r;
    return pg_backward(depth, n_ctx, d_t, d_v, pg_params(params, d_t, d_v), X, dG, dX, grads, pg_carve(workspace, depth, n_ctx, d_t, nullptr), (hipStream_t)stream);
}

// ---- the input pipeline on the device (augment.hip): stateless, no model handle.  Defined in this section so that the launcher-coverage
// check of tests/test_capi_cpu.py finds launch_augment behind an export; include/mudpt.h documents the three in a section of their own ----
extern "C" int mudpt_augment(const uint8_t* pixels_dev, const int64_t* images_dev, int32_t n_images, const int32_t* params_dev, int32_t batch, int32_t size,
                             const float* mean_std_host, float* out_dev, void* stream) {
    return launch_augment(pixels_dev, images_dev, n_images, params_dev, batch, size, mean_std_host, out_dev, (hipStream_t)stream);
}
extern "C" int mudpt_augment_check(const int64_t* images_host, int32_t n_images, const int32_t* params_host, int32_t batch, int32_t size) {
    ARG_CHECK(images_host && params_host, "augment_check: null argument");
    ARG_CHECK(n_images >= 0 && batch >= 0 && size >= 1, "augment_check: n_images %d, batch %d, size %d", n_images, batch, size);
    int64_t end = 0;  // first byte past the previous image
    for (int32_t i = 0; i < n_images; ++i) {
        const int64_t off = images_host[3 * i], H = images_host[3 * i + 1], W = images_host[3 * i + 2];
        ARG_CHECK(H >= 1 && H <= INT32_MAX, "augment_check: images row %d, column height = %lld: must be in [1, 2^31)", i, (long long)H);
        ARG_CHECK(W >= 1 && W <= INT32_MAX, "augment_check: images row %d, column width = %lld: must be in [1, 2^31)", i, (long long)W);
        ARG_CHECK(off >= end, "augment_check: images row %d, column offset = %lld: overlaps the image before it, which ends at byte %lld", i, (long long)off,
                  (long long)end);
        end = off + 3 * H * W;
    }
    static const char* const col[10] = {"image", "flip", "x_lo", "x_len", "x_out", "x_off", "y_lo", "y_len", "y_out", "y_off"};
    for (int32_t n = 0; n < batch; ++n) {
        const int32_t* p = params_host + (size_t)n * 10;
        ARG_CHECK(p[0] >= 0 && p[0] < n_images, "augment_check: params row %d, column %s = %d: outside [0, %d)", n, col[0], p[0], n_images);
        ARG_CHECK(p[1] == 0 || p[1] == 1, "augment_check: params row %d, column %s = %d: must be 0 or 1", n, col[1], p[1]);
        for (int a = 0; a < 2; ++a) {  // x: columns 2 .. 5 against the width, y: 6 .. 9 against the height
            const int32_t* q = p + 2 + 4 * a;
            const int64_t extent = images_host[3 * p[0] + (a == 0 ? 2 : 1)];
            ARG_CHECK(q[0] >= 0, "augment_check: params row %d, column %s = %d: must be >= 0", n, col[2 + 4 * a], q[0]);
            ARG_CHECK(q[1] >= 1 && (int64_t)q[0] + q[1] <= extent, "augment_check: params row %d, column %s = %d: needs 1 <= len and lo + len <= %lld", n,
                      col[3 + 4 * a], q[1], (long long)extent);
            ARG_CHECK(q[2] >= size, "augment_check: params row %d, column %s = %d: the output length must be >= size (%d)", n, col[4 + 4 * a], q[2], size);
            ARG_CHECK(q[3] >= 0 && (int64_t)q[3] + size <= q[2], "augment_check: params row %d, column %s = %d: needs 0 <= off and off + size (%d) <= out_len (%d)", n,
                      col[5 + 4 * a], q[3], size, q[2]);
        }
    }
    return MUDPT_OK;
}
extern "C" int mudpt_augment_form(int32_t x_len, int32_t x_out, int32_t y_len, int32_t y_out, int32_t size) { return augment_form(x_len, x_out, y_len, y_out, size); }

// ---- the ResNet tower's memory movers (resnet.hip) and the host-only weight packing its fold runs (include/mudpt.h lists the operands) ----
extern "C" int mudpt_im2col(int32_t dtype, const void* src, int32_t src_planar, int32_t B, int32_t H, int32_t W, int32_t C, int32_t lds, int32_t stride, void* dst,
                            int32_t ldk, void* stream) {
    return launch_im2col(dtype, src, src_planar != 0, B, H, W, C, lds, stride, dst, ldk, (hipStream_t)stream);
}
extern "C" int mudpt_conv2d(int32_t dtype, const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t lds, int32_t k, int32_t stride, const void* w,
                            int32_t ldk, const float* bias, const void* residual, int32_t ldres, void* out, int32_t ldo, int32_t N, int32_t relu, void* stream) {
    return launch_conv2d(dtype, src, B, H, W, C, lds, k, stride, w, ldk, bias, residual, ldres, out, ldo, N, relu != 0, (hipStream_t)stream);
}
extern "C" int mudpt_conv2d_form(int32_t M, int32_t N) { return conv2d_form(M, N); }
extern "C" int mudpt_bias_act(int32_t dtype, const float* acc, int32_t ldacc, const float* bias, const void* residual, int32_t ldres, void* out, int32_t ldo, int32_t M,
                              int32_t N, int32_t relu, void* stream) {
    return launch_bias_act(dtype, acc, ldacc, bias, residual, ldres, out, ldo, M, N, relu != 0, (hipStream_t)stream);
}
extern "C" int mudpt_avgpool2d(int32_t dtype, const void* src, int32_t lds, void* dst, int32_t ldo, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, void* stream) {
    return launch_avgpool2d(dtype, src, lds, dst, ldo, B, H, W, C, k, (hipStream_t)stream);
}
extern "C" int mudpt_attnpool_tokens(int32_t dtype, const void* src, int32_t lds, const float* pos, void* dst, int32_t ldo, int32_t B, int32_t HW, int32_t C, void* stream) {
    return launch_attnpool_tokens(dtype, src, lds, pos, dst, ldo, B, HW, C, (hipStream_t)stream);
}
extern "C" int mudpt_attnpool_attend(int32_t dtype, const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, void* out, int32_t ldo, int32_t B, int32_t L,
                                     int32_t H, void* stream) {
    return launch_attnpool_attend(dtype, q, ldq, k, v, ldkv, out, ldo, B, L, H, (hipStream_t)stream);
}
extern "C" int mudpt_conv_pack(int32_t dtype, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int32_t cout, int32_t cin, int32_t k,
                               int32_t ldk, void* w_out, float* bias_out) {
    ARG_CHECK(dtype == DT_BF16 || dtype == DT_F16, "conv_pack: unknown dtype %d", dtype);
    ARG_CHECK(w && gamma && beta && mean && var && w_out && bias_out, "conv_pack: null argument");
    ARG_CHECK(cout > 0 && cin > 0 && (k == 1 || k == 3) && ldk >= k * k * cin, "conv_pack: bad shape cout=%d cin=%d k=%d ldk=%d (k 1 | 3, ldk >= k k cin)", cout, cin, k, ldk);
    conv_pack(dtype, w, gamma, beta, mean, var, cout, cin, k, ldk, (uint16_t*)w_out, bias_out);
    return MUDPT_OK;
}

// ---- the text tower's sequence layout (plan_text_layout), host only ----
extern "C" int mudpt_text_layout_plan(const int32_t* eot, int32_t n_cls, int32_t ctx_len, int32_t n_prompt, int32_t heads, int32_t txt_trim, int32_t txt_buckets,
                                      int32_t txt_bucket_cost, int32_t allow_buckets, int32_t* cls, int32_t* first_row, int32_t* bucket_len, int32_t* buckets,
                                      int32_t* rows, int32_t* max_len) {
    ARG_CHECK(eot && cls && first_row && bucket_len && buckets && rows && max_len, "text_layout_plan: null argument");
    ARG_CHECK(n_cls >= 1 && heads >= 1, "text_layout_plan: n_cls %d and heads %d must be >= 1", n_cls, heads);
    ARG_CHECK(n_prompt >= 0 && n_prompt + 2 <= ctx_len, "text_layout_plan: n_prompt %d needs 0 <= n_prompt and n_prompt + 2 <= ctx_len (%d)", n_prompt, ctx_len);
    for (int32_t cc = 0; cc < n_cls; ++cc) ARG_CHECK(eot[cc] >= 0 && eot[cc] < ctx_len, "text_layout_plan: eot[%d] = %d outside [0, %d)", cc, eot[cc], ctx_len);
    TextLayout lay;
    const TextPlan p = plan_text_layout(eot, n_cls, ctx_len, n_prompt, heads, txt_trim != 0, txt_buckets, txt_bucket_cost, allow_buckets != 0, &lay);
    for (int32_t q = 0; q < n_cls; ++q) { cls[q] = p.order[q]; first_row[q] = p.first[q]; bucket_len[q] = lay.segs[p.seg[q]].L; }
    *buckets = (int32_t)lay.segs.size(); *rows = lay.rows; *max_len = lay.L;
    return MUDPT_OK;
}
