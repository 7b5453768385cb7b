/*
 * mudpt.h -- C ABI of libmudpt_hip.so, the MI355X (gfx950) implementation of the MuDPT prompt-tuning
 * hot path.  Plain pointers and sizes only; no torch / C++ types cross this boundary.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *   mudpt_create / mudpt_set_weight      clip/model.py:881-921 build_model + CLIP.__init__ :667-779
 *                                        (frozen weights ingested under OpenAI CLIP state-dict keys)
 *   mudpt_set_class_prompts              trainers/mudpt.py:83-95   token_prefix / token_suffix buffers,
 *                                        tokenized_prompts.argmax (EOT position, :154)
 *   mudpt_param_* / mudpt_bind_params    trainers/mudpt.py:205-218 the 10 trainable tensors (freeze rule)
 *   mudpt_forward                        trainers/mudpt.py:170-184 CustomCLIP.forward == model_inference()
 *   mudpt_forward_backward               trainers/mudpt.py:249-251 forward, F.cross_entropy, backward
 *   mudpt_sgd_step                       trainers/mudpt.py:251     model_backward_and_update's optimizer step
 *   mudpt_optim_step                     trainers/mudpt.py:225,251 the same step under any other OPTIM.NAME build_optimizer takes (adam, amsgrad, adamw, rmsprop)
 *   mudpt_allreduce_grads                trainers/mudpt.py:230-233 nn.DataParallel's gradient reduce (here: one RCCL all-reduce)
 *   mudpt_set_class_shard / mudpt_cp_*   trainers/mudpt.py:142-156,178-182 the same step with the class prompts divided over the ranks
 *   mudpt_gemm / _layernorm_* / _attention_*   the ATen ops under clip/model.py:164-175,257-301 (unit parity)
 *   mudpt_augment / _check / _form       configs/trainers/MuDPT/vit_b16_bz4_ep10_nctx2_depth9.yaml:9-13 INPUT.TRANSFORMS, INTERPOLATION "bicubic" (Dassl's transform pipeline on
 *                                        the loader's CPU workers) and trainers/mudpt.py:263-268 parse_batch_train's host -> device copy
 * With mudpt_config.variant = MUDPT_VARIANT_COCOOP the same entry points run the CoCoOp path (trainers/cocoop.py):
 *   mudpt_create / mudpt_set_weight      trainers/cocoop.py:22-40  load_clip_to_cpu: vanilla CLIP (clip/model.py:443-496 ViT)
 *   mudpt_set_class_prompts              trainers/cocoop.py:113-122 token_prefix / token_suffix, tokenized_prompts
 *   mudpt_param_*                        trainers/cocoop.py:96-107,222-226  ctx + meta_net.linear1/2 (5 tensors)
 *   mudpt_forward                        trainers/cocoop.py:178-198 CustomCLIP.forward in eval mode (logits [B, C])
 *   mudpt_forward_backward               trainers/cocoop.py:196-197,258-261 cross-entropy inside forward + backward
 * With MUDPT_VARIANT_COOP / MUDPT_VARIANT_COOP_CSC they run the CoOp path (trainers/coop.py):
 *   mudpt_create / mudpt_set_weight      trainers/coop.py:20-37    load_clip_to_cpu: vanilla CLIP, vision tower forward only
 *   mudpt_set_class_token_position       trainers/coop.py:78-97    name_lens, CLASS_TOKEN_POSITION
 *   mudpt_set_class_prompts              trainers/coop.py:85-93,99-164  token_prefix / token_suffix, construct_prompts' row order
 *   mudpt_param_*                        trainers/coop.py:60-76    ctx [n_ctx, d_t] (shared) or [n_cls, n_ctx, d_t] (CSC): 1 tensor
 *   mudpt_forward / _ex                  trainers/coop.py:212-226  CustomCLIP.forward (logits [B, C])
 *   mudpt_forward_backward               trainers/coop.py:281-296  forward, F.cross_entropy, backward w.r.t. ctx
 * With MUDPT_VARIANT_VPT / MUDPT_VARIANT_MPT (created by mudpt_create_ex) they run the deep-prompt baselines (trainers/vpt.py, mpt.py):
 *   mudpt_create_ex                      clip/model.py:404-416,443-470,752-770  per-tower prompt counts and depths (mudpt_prompt_shape)
 *   mudpt_set_class_prompts              trainers/vpt.py:43-70, mpt.py:43-125  "<TEXT_CTX_INIT> <name>." (MPT: rows 1..n_t replaced)
 *   mudpt_param_*                        clip/model.py:202-251,459-465, mpt.py:86  every "visual_ctx" [n, width], in named_parameters() order
 *   mudpt_forward / _ex                  trainers/vpt.py:94-111, mpt.py:156-172    CustomCLIP.forward (logits [B, C])
 *   mudpt_forward_backward               trainers/vpt.py:168-200, mpt.py:224-256   forward, F.cross_entropy, backward w.r.t. the prompts
 *   (VPT: the text tower has nothing to learn; its features are computed once per handle and reused until mudpt_set_weight /
 *    mudpt_set_class_prompts.  mudpt_set_class_shard, mudpt_cp_* and mudpt_set_class_token_position refuse both variants.)
 * With MUDPT_VARIANT_UMUDPT they run the unified prompt generator's path (trainers/umudpt.py; the towers are MuDPT's, clip/model.py:304-351,556-597):
 *   mudpt_create                         trainers/umudpt.py:83-92  TRAINER.UMUDPT.N_CTX (1..16) / DEEP_PROMPT_DEPTH (> 0) as n_ctx / depth
 *   mudpt_set_class_prompts              trainers/umudpt.py:126-133 token_prefix / token_suffix, tokenized_prompts
 *   mudpt_param_*                        trainers/umudpt.py:110-124,252-255  the 20 "umudpt_prompt_learner.*" tensors: ctx, deep_prompts
 *                                        ([depth - 1, n_ctx, d_t]: listed with 0 elements at depth 1), ln_pre, self_attn.{attn, ln_1, mlp, ln_2},
 *                                        ln_post, visual_proj, in named_parameters() order
 *   mudpt_forward / _ex                  trainers/umudpt.py:161-178,217-230  G = visual_proj(ln_post(Block(ln_pre(cat(ctx, deep_prompts))))) in fp32;
 *                                        G[0] = the vision tower's input prompt rows, G[1:] its deep prompts; the text tower takes ctx /
 *                                        deep_prompts as they are.  MUDPT_FWD_REUSE_TEXT keeps G as well as the text features.
 *   mudpt_forward_backward               trainers/umudpt.py:292-294  forward, F.cross_entropy, backward w.r.t. all 20 tensors
 *   (mudpt_set_class_shard, mudpt_cp_* and mudpt_set_class_token_position refuse the variant.)
 * With MUDPT_VARIANT_UUMUDPT they run the path with a generator in either direction (trainers/uumudpt.py; clip/model.py:600-664):
 *   mudpt_create                         trainers/uumudpt.py:84-93  TRAINER.UUMUDPT.N_CTX (1..16) / DEEP_PROMPT_DEPTH (> 0); embed_dim must equal t_width (:224)
 *   mudpt_param_*                        trainers/uumudpt.py:111-125,255-261, clip/model.py:606-628  40 tensors: UMuDPT's 20 as "uumudpt_prompt_learner.*",
 *                                        then the vision tower's "image_encoder.visual_ctx" [n_ctx, d_v], "visual_ctx_deep_prompts" [depth - 1, n_ctx, d_v]
 *                                        and its own generator "visual_ctx_{ln_intra_pre, self_attn.*, ln_intra_post, text_proj}" (width d_v, output e)
 *   mudpt_forward / _ex                  trainers/uumudpt.py:162-180,219-233  G = Gen1(cat(ctx, deep_prompts)); vision input rows G[0] + visual_ctx, vision deep
 *                                        prompts G[1:] + visual_ctx_deep_prompts; text deep prompts deep_prompts + Gen2(visual_ctx_deep_prompts); text
 *                                        input rows ctx.  Gen2 runs on the text stream beside Gen1 and idles at depth 1.  MUDPT_FWD_REUSE_TEXT keeps
 *                                        all of it: every one is a function of the parameters alone.
 *   mudpt_forward_backward               trainers/uumudpt.py:295-297  forward, F.cross_entropy, backward w.r.t. all 40 tensors
 *   (mudpt_set_class_shard, mudpt_cp_* and mudpt_set_class_token_position refuse the variant.)
 * A handle made by mudpt_create_frozen runs the zero-shot baselines (trainers/zsclip.py; lpclip/feat_extractor.py): CLIP as it was trained, nothing to learn:
 *   mudpt_create_frozen / mudpt_set_weight   trainers/zsclip.py:10-29  load_clip_to_cpu: vanilla CLIP, both towers forward only (clip/model.py:443-496,825-838);
 *                                        "token_embedding.weight" stays on the device
 *   mudpt_set_text_tokens                trainers/zsclip.py:61-65,108-110  clip.tokenize(template.format(classname)) for every template and class;
 *                                        clip/model.py:827,836  token_embedding(text) + positional_embedding, text.argmax(dim=-1)
 *   mudpt_text_features                  trainers/zsclip.py:67-71 (one template: f / |f|), :107-117 (ensemble: normalise, mean over the templates, normalise)
 *   mudpt_encode_image                   clip/model.py:822 encode_image, lpclip/feat_extractor.py:125  the raw visual(image) features
 *   mudpt_forward / _ex                  trainers/zsclip.py:74-79  model_inference: logit_scale * normalise(image features) @ text_features.t()
 *   (mudpt_param_count / _numel are 0; every training, class-prompt, class-shard and mudpt_cp_* entry point refuses the handle.)
 * A handle made by mudpt_create_frozen_resnet is such a frozen handle with CLIP's ResNet image tower (RN50, RN101, RN50x16, RN50x64; the backbone
 * of the zero-shot and linear-probe baselines, scripts/zsclip/run_zsclip.sh:15, lpclip/feat_extractor.py:113-116); the text side is the same:
 *   mudpt_create_frozen_resnet / mudpt_set_weight   clip/model.py:686-694, 890-897  build_model's ResNet branch; the "visual.*" keys of ModifiedResNet
 *   mudpt_encode_image / mudpt_forward / _ex         clip/model.py:17-161  ModifiedResNet.forward in eval mode: the stem, four stages of Bottleneck,
 *                                        AttentionPool2d; BatchNorm folded into the convolutions, every convolution an im2col + MFMA GEMM
 * A handle made by mudpt_create_resnet trains CoOp / CoCoOp on that tower (the backbone of CoOp's few-shot tables, scripts/coop/main.sh): the rows of
 * MUDPT_VARIANT_COOP / _COOP_CSC / _COCOOP above with ModifiedResNet as the frozen image encoder:
 *   mudpt_create_resnet / mudpt_set_weight           trainers/coop.py:20-37, cocoop.py:22-40  load_clip_to_cpu with an RN* backbone
 *   mudpt_forward / _ex / mudpt_forward_backward     trainers/coop.py:212-226,281-296, cocoop.py:178-198  the tower forward only, no image gradient
 * Frozen, CoOp and CoCoOp handles also run the test pass from cached image features:
 *   mudpt_forward_features               trainers/zsclip.py:74-79, coop.py:212-223, cocoop.py:178-188 behind their clip_model.visual(image)
 *   mudpt_image_features                 lpclip/feat_extractor.py:125-137  the features of the last inference forward, for {dir}/{dataset}/{split}.npz
 * The linear probe (lpclip/linear_probe.py:64, sklearn's LogisticRegression(solver="lbfgs")) needs no handle: its objective is evaluated by the
 * stateless mudpt_probe_* kernels at the end of this file, and mudpt_amd/lpclip.py + mudpt_amd/lbfgs.py drive them.
 * The test pass's evaluator (Dassl's evaluation/evaluator.py Classification, the end of every script's trainer.test()) needs none either: the
 * stateless mudpt_eval_* four at the end of this file count on the device, and mudpt_amd/evaluator.py drives them.
 *
 * Conventions: every function returns 0 on success or a MUDPT_ERR_* code; mudpt_last_error() gives
 * the message of the calling thread's last failure.  No exceptions cross the ABI.  A model handle is
 * not re-entrant.  Device pointers are HIP device memory owned by the caller unless stated; `stream`
 * is a hipStream_t passed as void* (NULL = default stream).  All launches are asynchronous.
 */
#ifndef MUDPT_H
#define MUDPT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 7 still with mudpt_create_frozen, mudpt_set_text_tokens, mudpt_text_features, mudpt_encode_image, the mudpt_augment* three and mudpt_optim_step: they are additions, no existing
 * declaration, struct or constant changed, so every caller built against 7 runs unchanged -- the number moves when one would not.
 * mudpt_amd/capi.py binds from this file: it parses every declaration (int / int32_t / int64_t / float / size_t, const char*, any other pointer
 * or array; a type outside that raises at import) and every integer #define MUDPT_*, so names, types and order are stated here only. */
#define MUDPT_ABI_VERSION 7

#define MUDPT_OK 0
#define MUDPT_ERR_ARG 1   /* bad argument / shape (the reference raises AssertionError, mudpt.py:52,55,190) */
#define MUDPT_ERR_HIP 2   /* a HIP runtime call failed */
#define MUDPT_ERR_STATE 3 /* call order: weights / prompts / parameters not set yet */

#define MUDPT_BF16 0
#define MUDPT_F16 1
/* The PARITY mode, what PREC = "fp32" selects (the reference's CPU path is fp32 whatever PREC says: clip/clip.py:142-143): the mode that
 * holds north_star's bound -- logits within 1e-3 of the reference -- at the logit scale pretrained checkpoints carry (exp(logit_scale) =
 * 100, trainers/mudpt.py:181).  fp16 MFMA operands with SPLIT forward GEMM operands (hi = fp16(v) plus the remainder, contracted in a
 * second pass against the fp16-exact weights, as CLIP checkpoints store them):
 *   text tower    remainder as fp16 (22 bits) + attention forward in fp32 on the matrix cores (v_mfma_f32_16x16x4_f32): each of its
 *                 rounding sites alone moves the logits by 2.5e-3;
 *   vision tower  remainder as e4m3, contracted against an e4m3 copy of the weights on the MX-scaled fp8 matrix instruction
 *                 (v_mfma_scale_f32_16x16x128_f8f6f4: twice the fp16 rate, so the second pass costs half of the first), pixels included;
 *                 attention in fp16.
 * Measured against the reference's own logits at scale 100: <= 3.5e-4 (ViT-B/16; 1.2e-4 ViT-L/14@336), 1.26x the bf16 step.  Knobs
 * (mudpt_model_set): vis_exact_attn = 1 -> 8e-5; vis_lo = 1 + vis_exact_attn = 1 -> round 3's "exact" mode, 2e-5 at 1.6x.  The
 * backward is the MUDPT_F16 one with fp16 activation gradients.  Per-site ablation: DESIGN.md 2. */
#define MUDPT_F32 2

#define MUDPT_VARIANT_MUDPT 0  /* trainers/mudpt.py: deep multi-modal prompts, 10 trainables */
#define MUDPT_VARIANT_COCOOP 1 /* trainers/cocoop.py: instance-conditioned text prompts, 5 trainables; depth is ignored */
#define MUDPT_VARIANT_COOP 2     /* trainers/coop.py: one shared context [n_ctx, t_width], the trainable "prompt_learner.ctx"; depth is ignored */
#define MUDPT_VARIANT_COOP_CSC 3 /* trainers/coop.py with CSC: one context per class, [n_cls, n_ctx, t_width]; depth is ignored */
#define MUDPT_VARIANT_VPT 4      /* trainers/vpt.py: deep vision prompts only; mudpt_create_ex, n_ctx / depth are ignored */
#define MUDPT_VARIANT_MPT 5      /* trainers/mpt.py: independent deep prompts in each tower; mudpt_create_ex, n_ctx / depth are ignored */
#define MUDPT_VARIANT_UMUDPT 6   /* trainers/umudpt.py: MuDPT's towers, the vision prompts GENERATED from the text prompts by a trainable block; 20 trainables */
#define MUDPT_VARIANT_UUMUDPT 7  /* trainers/uumudpt.py: UMuDPT plus a second generator, vision deep prompts -> an addend of the text deep prompts; 40 trainables */

/* CoOp's TRAINER.COOP.CLASS_TOKEN_POSITION (trainers/coop.py:99-164): where the class-name tokens sit relative to the context rows */
#define MUDPT_CLASS_TOKEN_END 0    /* [SOS, ctx, name, ".", EOT]                        (default) */
#define MUDPT_CLASS_TOKEN_MIDDLE 1 /* [SOS, ctx[:n/2], name, ctx[n/2:], ".", EOT]        (n/2 rounds down) */
#define MUDPT_CLASS_TOKEN_FRONT 2  /* [SOS, name, ctx, ".", EOT] */

/* Model shape.  ViT-B/16 MuDPT: {224,16,768,12,12, 512,12,8,77, 512, 4,12, n_cls, max_batch, dtype, 0}. */
typedef struct mudpt_config {
    int32_t image_size, patch, v_width, v_layers, v_heads;
    int32_t t_width, t_layers, t_heads, ctx_len;
    int32_t embed_dim;
    int32_t n_ctx, depth; /* TRAINER.MUDPT.N_CTX / DEEP_PROMPT_DEPTH (train.py:115-119) */
    int32_t n_cls;        /* number of class prompts */
    int32_t max_batch;    /* activations are sized for this many images */
    int32_t dtype;        /* MUDPT_BF16 / MUDPT_F16: MFMA operand type (fp32 accumulate, fp32 residual stream); MUDPT_F32: the parity mode */
    int32_t variant;      /* MUDPT_VARIANT_*; CoCoOp runs max_batch * n_cls text sequences per step */
} mudpt_config;

typedef struct mudpt_model mudpt_model;

int mudpt_abi_version(void);
const char* mudpt_last_error(void);

int mudpt_create(const mudpt_config* cfg, mudpt_model** out);  /* VPT / MPT: MUDPT_ERR_ARG, use mudpt_create_ex */

/* VPT / MPT prompt shape, TRAINER.<NAME>.* (train.py:98-113).  Vision: visual_ctx [v_n_ctx, v_width] appended after the positional
 * embedding and before ln_pre, and blocks 1 <= i < v_depth replace the last v_n_ctx rows with their own visual_ctx -- only if
 * 0 < v_depth <= 12 (clip/model.py:459); any other depth is the vanilla ViT, which then runs forward only.  Text (MPT): the
 * text_prompt_learner's visual_ctx [t_n_ctx, t_width] takes rows 1..t_n_ctx of every class prompt (with the positional embedding,
 * trainers/mpt.py:108-125), and blocks 1 <= i < min(t_depth, t_layers) replace those rows with their own visual_ctx (no cap).
 * Refused (MUDPT_ERR_ARG, before any GPU call): VPT without a vision prompt (nothing to train), VPT with text deep prompts
 * (t_n_ctx > 0 and t_depth > 1), MPT with t_n_ctx < 1. */
typedef struct mudpt_prompt_shape {
    int32_t t_n_ctx, t_depth; /* TRAINER.<NAME>.DEEP_TEXT_N_CTX / TEXT_PROMPT_DEPTH */
    int32_t v_n_ctx, v_depth; /* TRAINER.<NAME>.DEEP_VISUAL_N_CTX / VISUAL_PROMPT_DEPTH */
} mudpt_prompt_shape;
/* mudpt_create for every variant: prompts = NULL for MuDPT / CoCoOp / CoOp (then identical to mudpt_create), required for VPT / MPT. */
int mudpt_create_ex(const mudpt_config* cfg, const mudpt_prompt_shape* prompts, mudpt_model** out);
/* Frozen CLIP (trainers/zsclip.py): both towers vanilla and forward only, no trainable tensor.  cfg->variant, n_ctx and depth are not read;
 * n_cls, max_batch, dtype (all three) and the shape fields are what they are for mudpt_create.  The handle takes mudpt_set_weight (and keeps
 * "token_embedding.weight" on the device as fp32 [vocab, t_width], vocab = numel / t_width), mudpt_set_text_tokens, mudpt_text_features,
 * mudpt_encode_image, mudpt_forward / _ex (MUDPT_FWD_REUSE_TEXT accepted, no effect: the text features are always kept), mudpt_text_layout,
 * mudpt_model_set, mudpt_debug_read ("image_features", "text_features" = the ensembled, normalised table, "text_launches") and mudpt_destroy.
 * mudpt_param_count / _numel return 0; mudpt_bind_params, mudpt_forward_backward, mudpt_sgd_step, mudpt_set_class_prompts,
 * mudpt_set_class_token_position, mudpt_set_class_shard, mudpt_cp_* and mudpt_allreduce_grads return MUDPT_ERR_ARG ("... frozen ..."). */
int mudpt_create_frozen(const mudpt_config* cfg, mudpt_model** out);
/* Frozen CLIP with the ResNet image tower ModifiedResNet(layers, embed_dim, heads, image_size, width) (clip/model.py:101-161, built by
 * clip/model.py:686-694 whenever a checkpoint has no "visual.proj", :890-897).  A frozen handle in everything else: the text side
 * (mudpt_set_text_tokens, mudpt_text_features, the ensembling), mudpt_encode_image, mudpt_forward / _ex, mudpt_forward_features,
 * mudpt_image_features and mudpt_debug_read("image_features") are what they are for mudpt_create_frozen.  Read from cfg: image_size, embed_dim,
 * n_cls, max_batch, dtype and the text shape; NOT read: patch, v_width, v_layers, v_heads, n_ctx, depth, variant.  embed_dim need not equal
 * t_width (RN50: 1024 / 512).  Activations are NHWC in T, sized here for max_batch; BatchNorm (eval mode, eps 1e-5) is folded into the
 * convolution weights on the host, in fp64, at the first forward after a "visual.*" upload (mudpt_conv_pack below is that function).
 * MUDPT_ERR_ARG before any GPU call, the message naming the field: a null pointer; image_size % 32 != 0; a stage count < 1; width % 32 != 0
 * (RN50x4, width 80: its 40-channel stem does not meet the GEMM's N % 16); heads < 1 or (32 width) % heads != 0; (32 width) / heads != 64, the
 * head dimension of every released model (clip/model.py:687); dtype MUDPT_F32 ("ResNet towers run in bf16 / fp16; the parity mode is not built
 * for them").
 * mudpt_set_weight takes the reference's keys, shapes checked against this shape: visual.conv{1,2,3}.weight (conv1 is [width / 2, 3, 3, 3]),
 * visual.bn{1,2,3}.{weight,bias,running_mean,running_var}, visual.layer{1..4}.{i}.{conv1,bn1,conv2,bn2,conv3,bn3}.*,
 * visual.layer{1..4}.0.downsample.{0.weight,1.*}, visual.attnpool.positional_embedding, visual.attnpool.{q,k,v,c}_proj.{weight,bias};
 * "*.num_batches_tracked" is accepted and ignored.  The entry points that run the tower return MUDPT_ERR_STATE naming the first missing key
 * until all of them are there; mudpt_forward_features and mudpt_text_features need none of them. */
typedef struct mudpt_resnet_shape {
    int32_t layers1, layers2, layers3, layers4; /* Bottleneck blocks per stage: RN50 3, 4, 6, 3; RN101 3, 4, 23, 3 */
    int32_t width;                              /* 64 (RN50, RN101), 96 (RN50x16), 128 (RN50x64); the tower's output has 32 width channels */
    int32_t heads;                              /* of the attention pool: 32 width / 64 */
} mudpt_resnet_shape;
int mudpt_create_frozen_resnet(const mudpt_config* cfg, const mudpt_resnet_shape* rn, mudpt_model** out);
/* A TRAINABLE handle with that tower: what mudpt_create makes for MUDPT_VARIANT_COOP, _COOP_CSC and _COCOOP, the image tower set up as
 * mudpt_create_frozen_resnet sets it up.  Both trainers keep the image encoder frozen and prompt-free (trainers/coop.py:212-226,
 * cocoop.py:178-198), so the tower runs forward only where the vanilla ViT would; embed_dim need not equal t_width, CoCoOp's meta_net keeps
 * its hidden width embed_dim / 16 (cocoop.py:104).  Read from cfg: image_size, embed_dim, n_ctx, n_cls, max_batch, dtype, variant and the text
 * shape; NOT read: patch, v_width, v_layers, v_heads, depth.  Everything a ViT CoOp / CoCoOp handle takes, this one takes: mudpt_set_weight
 * ("visual.*": the keys above, folded and refolded as above), mudpt_set_class_prompts, mudpt_set_class_token_position, mudpt_bind_params,
 * mudpt_forward / _ex, mudpt_forward_backward, mudpt_forward_features, mudpt_image_features, mudpt_sgd_step.  The training head asks for no
 * image gradient (mudpt_head_ex with dimg = NULL), and neither that buffer nor any ViT block activation is allocated.
 * MUDPT_ERR_ARG before any GPU call: any other variant ("... its prompts live inside a ViT ..."), and everything
 * mudpt_create_frozen_resnet refuses, in the same words. */
int mudpt_create_resnet(const mudpt_config* cfg, const mudpt_resnet_shape* rn, mudpt_model** out);
/* How a ResNet handle (either of the two above) runs the convolutions of its tower.  path 0, the default: every convolution is patch rows
 * (mudpt_im2col; a 1 x 1 reads the activation as it lies) + the GEMM with an fp32 output + mudpt_bias_act.  path 1: every convolution of the
 * stem, the Bottlenecks and the downsample branches is ONE mudpt_conv2d launch, the residual of conv3 in its epilogue; the stem's first
 * convolution (fp32 planar pixels, 3 channels) keeps its patch rows and runs mudpt_conv2d over them as a 1 x 1.  The poolings and the
 * attention pool are the same launches.  Both paths round at the same places (mudpt_amd/csrc/resnet.hip lists them), so both are held to the
 * same bounds; their bits differ where the fp32 sums run in another order.  May be called between any two forwards; an addition, so
 * MUDPT_ABI_VERSION stays.  The buffers of path 0 stay allocated on path 1.
 * MUDPT_ERR_ARG with a message: a null handle; a handle without a ResNet tower ("... has no ResNet image tower ..."); a path outside {0, 1}. */
int mudpt_resnet_conv_path(mudpt_model* m, int32_t path);
int mudpt_destroy(mudpt_model* m);

/* Frozen weight by OpenAI CLIP state-dict key ("visual.transformer.resblocks.0.attn.in_proj_weight", ...),
 * fp32 HOST data in the checkpoint's own layout; the library converts / transposes to its device layout.
 * Keys the path does not use ("token_embedding.weight", ...) are accepted and ignored; a frozen handle (mudpt_create_frozen) keeps
 * "token_embedding.weight". */
int mudpt_set_weight(mudpt_model* m, const char* key, const float* host_data, size_t numel);

/* token_embedding(tokenized "<ctx words> <classname>.") [n_cls, ctx_len, t_width] fp32 HOST and the EOT
 * position of every class prompt; rows 1..n_ctx are replaced by the trainable ctx at run time.  The text tower then runs on
 * positions 0..max(eot_index) only: under the causal mask (clip/model.py:407-413) later positions reach neither the EOT
 * feature (trainers/mudpt.py:154) nor any gradient. */
int mudpt_set_class_prompts(mudpt_model* m, const float* embedding, const int32_t* eot_index);
/* Frozen handles only: the class prompts as token ids, tokens [n_templates, n_cls, ctx_len] int32 HOST = clip.tokenize(template t formatted
 * with class c); the EOT position of a prompt is the first index of its row's maximum (text.argmax(dim=-1), clip/model.py:836).  Every
 * template gets its own text layout by the rules of mudpt_set_class_prompts (trim to its longest EOT, length buckets; the knobs txt_trim,
 * txt_buckets, txt_bucket_cost are read here) and two int32 device tables with the token id and the position of every packed token row; the
 * embedding is looked up on the device.  Activations are sized for the largest template.  The text features -- normalise(f) for one
 * template, normalise(mean_t normalise(f_t)) for more, templates in ascending order (bit-reproducible) -- are computed at the next
 * mudpt_forward / _ex / mudpt_text_features and kept until the next mudpt_set_weight or mudpt_set_text_tokens.  MUDPT_ERR_ARG before any GPU
 * call: a null pointer, n_templates < 1, an id outside [0, vocab), not a frozen handle; MUDPT_ERR_STATE: "token_embedding.weight" or
 * "positional_embedding" not set yet.  mudpt_text_layout then reports the token rows summed over the templates, the largest bucket count
 * of a template and the longest kept length. */
int mudpt_set_text_tokens(mudpt_model* m, const int32_t* tokens, int32_t n_templates);
/* Frozen handles only: copies the [n_cls, embed_dim] text features (fp32, rows of norm 1) to feat_dev, computing them first if a weight or
 * the tokens changed since; asynchronous on `stream`. */
int mudpt_text_features(mudpt_model* m, float* feat_dev, void* stream);
/* Frozen handles only: features_dev [batch, embed_dim] fp32 = visual(image), RAW (not normalised), for images_dev [batch, 3, S, S] fp32.
 * Needs the weights only, not the tokens. */
int mudpt_encode_image(mudpt_model* m, const float* images_dev, int32_t batch, float* features_dev, void* stream);
/* CoOp handles only (any other handle: MUDPT_ERR_ARG), before mudpt_set_class_prompts.  position = MUDPT_CLASS_TOKEN_*; name_lens [n_cls]
 * HOST = len(_tokenizer.encode(name)) of every class (trainers/coop.py:80), may be NULL for MUDPT_CLASS_TOKEN_END.  mudpt_set_class_prompts
 * still receives token_embedding("<X ... X> <name>.") in tokenized order and reorders the rows itself; it refuses a class unless
 * 0 <= name_lens[c] and 1 + n_ctx + name_lens[c] <= eot_index[c]. */
int mudpt_set_class_token_position(mudpt_model* m, int32_t position, const int32_t* name_lens);
/* What the text tower runs per pass after mudpt_set_class_prompts: token rows, length buckets, longest kept length.  With many classes
 * (>= 2048 rows) the prompts are sorted by length and run in up to "txt_buckets" (mudpt_model_set, default 3) groups, each to its own
 * longest EOT, instead of all to the overall longest: the kept rows are bit-identical, the padding rows are not computed. */
int mudpt_text_layout(const mudpt_model* m, int32_t* rows, int32_t* buckets, int32_t* max_len);

/* The 10 trainable tensors live in ONE flat fp32 bucket (= the data-parallel all-reduce payload). */
int mudpt_param_count(const mudpt_model* m);   /* 10 (MuDPT), 5 (CoCoOp), 1 (CoOp), 1 + vision blocks (VPT) or that + 1 + text blocks (MPT), 20 (UMuDPT), 40 (UUMuDPT) */
size_t mudpt_param_numel(const mudpt_model* m); /* elements of the flat bucket */
/* name = the reference's CustomCLIP state-dict key; shape has ndim entries (ndim <= 3). */
int mudpt_param_info(const mudpt_model* m, int index, const char** name, size_t* offset, size_t* numel,
                     int32_t* ndim, int64_t shape[3]);
/* Device pointers to the flat parameter bucket and the flat gradient bucket (caller-owned, fp32). */
int mudpt_bind_params(mudpt_model* m, float* params_dev, float* grads_dev);

/* logits[B, n_cls] fp32 for images[B,3,S,S] fp32 (CLIP-normalised pixels), both device memory. */
int mudpt_forward(mudpt_model* m, const float* images_dev, int32_t batch, float* logits_dev, void* stream);

/* Same with flags.  MUDPT_FWD_REUSE_TEXT: keep the text features of the previous call (valid while the bound parameters
 * are unchanged): the reference recomputes the text tower for every test batch (trainers/mudpt.py:170-184). */
#define MUDPT_FWD_REUSE_TEXT 1
/* mudpt_cp_forward only: this forward is the first phase of a TRAINING step (mudpt_forward_backward implies it).  A training forward may
 * split the contraction of the vision tower's out_proj / c_proj at tiny batches (<= 8 ViT-B images; a differently associated fp32 sum);
 * an inference forward never does, so the logits of an image do not depend on the size of the test batch it arrives in. */
#define MUDPT_FWD_TRAINING 2
int mudpt_forward_ex(mudpt_model* m, const float* images_dev, int32_t batch, float* logits_dev, int32_t flags, void* stream);

/* The test pass from cached image features (additions: MUDPT_ABI_VERSION stays).  trainers/zsclip.py:74-79 (ZeroshotCLIP / ZeroshotCLIP2),
 * trainers/coop.py:212-223 (CoOp) and trainers/cocoop.py:178-188 (CoCoOp) all begin with the frozen, prompt-free clip_model.visual(image) and
 * read nothing else of the image: per image that call is a constant, and lpclip/feat_extractor.py:125-137 names the file that holds it
 * ({dir}/{dataset}/{split}.npz).  mudpt_forward_features is mudpt_forward_ex with that call replaced by its result: features_dev
 * [batch, embed_dim] fp32, RAW (not normalised) -- what mudpt_encode_image and mudpt_image_features return -- is copied to where the
 * vision tower leaves its output, and everything behind it runs through the same code: a frozen handle computes its text features if a
 * weight or the tokens changed and runs the logits-only head (it needs no "visual.*" weight for this, nor does mudpt_text_features); CoOp runs the text tower, unless
 * MUDPT_FWD_REUSE_TEXT, and the head; CoCoOp normalises, runs meta_net, the per-image prompts, the chunked text tower and the pair head.
 * Logits of forwarded features equal the logits of the image forward they came from bit for bit, under any chunking of the batch.
 * MUDPT_ERR_ARG, nothing launched and the handle as it was: MuDPT, VPT, MPT, UMuDPT, UUMuDPT (their trainable prompts run inside the vision
 * tower, so their image features are no constant), a null pointer, batch outside 1..max_batch; MUDPT_ERR_STATE as mudpt_forward_ex. */
int mudpt_forward_features(mudpt_model* m, const float* features_dev, int32_t batch, float* logits_dev, int32_t flags, void* stream);
/* The raw visual(image) features [batch, embed_dim] of the last INFERENCE forward (mudpt_forward / _ex, mudpt_forward_features,
 * mudpt_encode_image) of a frozen, CoOp or CoCoOp handle, device to device, asynchronous on `stream`: what lpclip/feat_extractor.py:125
 * appends per batch, taken from a test pass that ran anyway.  MUDPT_ERR_STATE: no such forward since the handle was created or since a
 * training step, or it had another batch size; MUDPT_ERR_ARG: the five variants mudpt_forward_features refuses, a null pointer. */
int mudpt_image_features(mudpt_model* m, int32_t batch, float* features_dev, void* stream);

/* One training step's forward + backward: loss_dev[0] = mean cross-entropy over the batch, gradients of
 * (grad_scale * loss) written to the bound gradient bucket.  logits_dev may be NULL.  grad_scale = 1/world
 * makes the sum over data-parallel ranks the gradient of the global-batch mean. */
int mudpt_forward_backward(mudpt_model* m, const float* images_dev, const int64_t* labels_dev, int32_t batch,
                           float grad_scale, float* loss_dev, float* logits_dev, void* stream);

/* The step split at the head, for a loss of the caller's (additions: MUDPT_ABI_VERSION stays).  The reference's CustomCLIP.forward returns
 * logits (trainers/mudpt.py:170-184) and the loss is one line of forward_backward (:249-251) that anyone can change; here
 *   mudpt_forward_train(images)        the first half of mudpt_forward_backward: both towers as a TRAINING forward, the logits-only head;
 *                                      logits_dev [batch, n_cls] fp32
 *   mudpt_train_features(...)          the RAW (un-normalised) features of that forward, device to device: image_features_dev [batch, embed_dim],
 *                                      text_features_dev [n_cls, embed_dim]; either may be NULL
 *   <the caller's loss L and its gradients with respect to the three tensors>
 *   mudpt_backward_logits(dL/dlogits, dL/dimage_features, dL/dtext_features)   the second half: the bucket is zeroed and receives the gradient of
 *                                      (grad_scale * L).  Any of the three may be NULL (not all).  The head's backward from the given gradients
 *                                      (mudpt_head_grad with gmul = loss_scale * batch, so for L = mean cross-entropy the towers see the logit gradients
 *                                      mudpt_forward_backward forms itself), then that call's tail: VPT runs the vision side only, a vanilla vision
 *                                      tower the text side only; a ResNet handle accepts and ignores dimg_dev (nothing in front of its features trains).
 * All three are asynchronous on `stream`.  ONE forward feeds ONE backward: MUDPT_ERR_STATE from mudpt_train_features / mudpt_backward_logits if no
 * mudpt_forward_train with the same batch precedes, or if any other forward, step or a second backward came in between.  MUDPT_ERR_ARG before any
 * launch: a null model, a frozen handle, a class-sharded handle, CoCoOp (its step is chunked over the images and frees each chunk's text
 * activations before the next: all logits exist only after every backward would have had to start), a null images / logits pointer. */
int mudpt_forward_train(mudpt_model* m, const float* images_dev, int32_t batch, float* logits_dev, void* stream);
int mudpt_train_features(mudpt_model* m, int32_t batch, float* image_features_dev, float* text_features_dev, void* stream);
int mudpt_backward_logits(mudpt_model* m, const float* dlogits_dev, const float* dimg_dev, const float* dtxt_dev, int32_t batch, float grad_scale,
                          void* stream);
/* Which forward is in flight, for a host that keeps several results of mudpt_forward_train around (an autograd graph per call): every
 * mudpt_forward_train of a handle has a number, 1, 2, ...  mudpt_train_token writes the number of the one in flight to *token (may be NULL);
 * expect != 0: MUDPT_ERR_STATE unless that is the one in flight -- a later forward of the same batch size would otherwise take an earlier
 * forward's gradients.  MUDPT_ERR_STATE also when none is in flight.  mudpt_train_release ends the forward in flight without a backward (a
 * forward whose outputs are only read); none in flight: nothing happens.  mudpt_set_weight, mudpt_set_class_prompts and mudpt_bind_params end it too. */
int mudpt_train_token(mudpt_model* m, int64_t expect, int64_t* token);
int mudpt_train_release(mudpt_model* m);

/* Data parallelism (replaces nn.DataParallel, trainers/mudpt.py:230-233): one process per GPU, each computing the gradient of
 * (1/world) * local-mean loss (grad_scale above); the ONE exchange of a step is the sum of the flat gradient bucket over the ranks.
 * A host with torch.distributed does that itself (mudpt_amd/parallel.py: dist.all_reduce on the bound bucket); any other host
 * passes its RCCL communicator (ncclComm_t as void*, created with ncclCommInitRank) here.  In place on the bound bucket, asynchronous
 * on `stream`; RCCL is resolved from the process at first use (no link-time dependency). */
int mudpt_allreduce_grads(mudpt_model* m, void* nccl_comm, void* stream);

/* Class-parallel text tower: the second axis for many classes (ImageNet, C = 1000).  The reference replicates the text tower over all C
 * class prompts on every GPU (trainers/mudpt.py:142-156 inside nn.DataParallel, :230-233); here rank r may encode classes [c0, c1) only.
 * mudpt_set_class_shard comes before mudpt_set_class_prompts (which still receives ALL n_cls prompts on every rank and keeps its own).
 * A sharded handle refuses mudpt_forward / mudpt_forward_backward; one step is
 *   mudpt_cp_forward(images)        both towers; rows c0..c1-1 of feat[n_cls, embed] = this rank's text features, other rows zero
 *   exchange 1                      all-reduce(sum) -- or all-gather -- of feat over the ranks
 *   mudpt_cp_head(labels, ...)      logits / loss of the LOCAL images against ALL classes; backward -> dfeat[n_cls, embed]
 *                                   (labels NULL: inference, logits only, no exchange 2 / backward)
 *   exchange 2                      all-reduce(sum) of dfeat (every rank's images contribute to every class); it may overlap
 *   mudpt_cp_backward(MUDPT_CP_VISION)   ... the vision tower's backward, which does not read dfeat
 *   mudpt_cp_backward(MUDPT_CP_TEXT)     text tower backward over the local classes + prompt-learner backward, after exchange 2
 *   the gradient-bucket all-reduce  as in pure data parallelism (text-side gradients are partial sums over classes)
 * mudpt_cp_buffers returns the two fp32 device tables (library-owned, numel = n_cls * embed_dim).  Every phase is asynchronous on `stream`;
 * the caller orders its exchanges on that stream.  An unsharded handle may run the phases too (one rank: no exchange needed). */
#define MUDPT_CP_VISION 1
#define MUDPT_CP_TEXT 2
int mudpt_set_class_shard(mudpt_model* m, int32_t class_begin, int32_t class_end);
int mudpt_cp_buffers(mudpt_model* m, float** feat_dev, float** dfeat_dev, size_t* numel);
int mudpt_cp_forward(mudpt_model* m, const float* images_dev, int32_t batch, int32_t flags, void* stream);
int mudpt_cp_head(mudpt_model* m, const int64_t* labels_dev, int32_t batch, float grad_scale, float* loss_dev, float* logits_dev,
                  int32_t flags, void* stream);
int mudpt_cp_backward(mudpt_model* m, int32_t part, void* stream);

/* Static loss scale of the backward pass (default 128): per-sample logit gradients are multiplied by it so the
 * fp16 copies of the token gradients stay normal; the gradients written to the bucket are unscaled again.
 * Any positive finite value is accepted, a power of two or not; it takes effect at the next step (the class-parallel phases: at the next
 * mudpt_cp_head).  bf16 handles give the same step bit for bit at every power of two; fp16-typed handles keep their own gradient grade from
 * 1024 down to 2 and stay inside bf16's at 1, the floor of trainer.data_parallel_step (measured: the table in DESIGN.md 2).
 * The reference's analogue is GradScaler under PREC == "amp" (trainers/mudpt.py:228,243-246). */
int mudpt_set_loss_scale(mudpt_model* m, float loss_scale);

/* torch.optim.SGD update of the bound parameters from the bound gradients (momentum buffer library-owned). */
int mudpt_sgd_step(mudpt_model* m, float lr, float momentum, float weight_decay, float dampening,
                   int32_t nesterov, void* stream);
int mudpt_sgd_reset(mudpt_model* m);

/* The optimizer step for every OPTIM.NAME of Dassl's build_optimizer but "radam" (additions: MUDPT_ABI_VERSION stays): torch.optim.SGD, Adam
 * (amsgrad), AdamW and RMSprop (centered, momentum) by torch 2.10's single-tensor rules (torch/optim/adam.py::_single_tensor_adam, the
 * non-capturable branch; torch/optim/rmsprop.py::_single_tensor_rmsprop; the statements: mudpt_amd/csrc/optim.hip), ONE launch over the flat bucket.
 * The hyper-parameters are doubles, as torch's Python floats are: 1 - beta2, lr / (1 - beta1^step) and sqrt(1 - beta2^step) are formed in
 * double and rounded to fp32 once (1 - 0.999f would be 1.3e-5 off).  `step` is the 1-based count of THIS update, kept by the caller.
 * The state is CALLER-owned fp32 device memory of mudpt_param_numel elements per slot, zero before step 1 (a checkpoint is a copy of it):
 *   algo                  state[0]          state[1]                          state[2]
 *   MUDPT_OPTIM_SGD       momentum_buffer (momentum != 0; written, not read, at step 1)
 *   MUDPT_OPTIM_ADAM      exp_avg           exp_avg_sq                        max_exp_avg_sq (amsgrad)      L2 decay: grad + weight_decay param
 *   MUDPT_OPTIM_ADAMW     exp_avg           exp_avg_sq                        max_exp_avg_sq (amsgrad)      decoupled: param (1 - lr weight_decay)
 *   MUDPT_OPTIM_RMSPROP   square_avg        momentum_buffer (momentum > 0)    grad_avg (centered)
 * A slot the configuration does not use is not read and may be NULL.  Fields an algorithm does not use are not read either (SGD: lr, momentum,
 * weight_decay, dampening, nesterov; Adam / AdamW: lr, beta1, beta2, eps, weight_decay, amsgrad; RMSprop: lr, alpha, eps, weight_decay,
 * momentum, centered).  MUDPT_ERR_ARG before any GPU call: a null pointer, step < 1, eps <= 0, beta1 or beta2 outside [0, 1), a negative or
 * non-finite lr / weight_decay / alpha / momentum, a needed state slot that is NULL or (but for SGD) not 16-byte aligned, two buffers that
 * overlap, an unknown algo. */
#define MUDPT_OPTIM_SGD 0
#define MUDPT_OPTIM_ADAM 1
#define MUDPT_OPTIM_ADAMW 2
#define MUDPT_OPTIM_RMSPROP 3
typedef struct mudpt_optim {
    int32_t algo; /* MUDPT_OPTIM_* */
    double lr, beta1, beta2, eps, weight_decay, momentum, alpha, dampening;
    int32_t nesterov, amsgrad, centered;
    int64_t step; /* the 1-based count of this update */
    float* state[3];
} mudpt_optim;
/* Updates the bound parameters from the bound gradients (mudpt_bind_params); asynchronous on `stream`.  A frozen handle: MUDPT_ERR_ARG
 * ("... frozen ...").  It neither reads nor moves what mudpt_sgd_step keeps (its momentum buffer, its first-step flag). */
int mudpt_optim_step(mudpt_model* m, const mudpt_optim* optim, void* stream);

/* ======================================================================================================================================
 * Everything below this line is TEST / MEASUREMENT / DEBUG surface, not part of the drop-in boundary: a trainer plugin needs none of it.
 * ====================================================================================================================================== */

/* Test hook: copy an internal fp32 activation of the last call to HOST memory (synchronises the device).
 * name: "vis.x_in.<i>" / "txt.x_in.<i>" (input of block i, after the prompt splice; [seq, L, d], text L = max(eot) + 1), "vis.x_out" / "txt.x_out"
 * (output of the last block on the ONE row per sequence the model uses -- CLS / EOT token -- [seq, d]: the tail of the last
 * block runs on those rows only), "image_features", "text_features", "text_launches" (1 value: text-tower passes plus text-side head
 * launches -- normalisation of the text features, their gradient -- since the handle was created); UMuDPT: "umudpt.G" (the generator's output)
 * and "umudpt.dG" (its gradient as the vision tower's backward left it), each [depth, n_ctx, v_width]; UUMuDPT: "uumudpt.G" / "uumudpt.dG"
 * likewise and, at depth > 1, "uumudpt.T" (the second generator's output) / "uumudpt.dT" (its gradient as the text tower's backward left it),
 * each [depth - 1, n_ctx, embed_dim]; a ResNet handle: "conv2d_launches" (1 value: the mudpt_conv2d launches of its tower since the handle was
 * created -- mudpt_resnet_conv_path 0 adds none, path 1 one per convolution).  host_out may be NULL to query *numel. */
int mudpt_debug_read(mudpt_model* m, const char* name, int32_t batch, float* host_out, size_t capacity, size_t* numel);

/* Debug knobs of ONE handle, for A/B measurements in one process and for tests (tools/gemm_bench.py, bench.py flags, tests/).  Nothing is
 * process-global: two models in one process do not interfere.  Defaults are what the product runs; no knob is needed for correct results.
 *
 *   knob               default         meaning
 *   gemm_variant       0               kernel choice of the MFMA GEMMs (gemm.hip launch_epi / gemm_pp.hip; 0 = the default dispatch; 12 = the default
 *                                      without the 128-deep K-tiles of the small grids; other values force one tile form: A/B runs)
 *   split_k            1               0 = never split the contraction of the vision tower's small-grid, long-K store GEMMs
 *   fwd_split_k        1               0 = ... of the forward ones (out_proj / c_proj up to 320 tiles of 64 x 64, i.e. <= 8 images of ViT-B): logits
 *                                      of a batch then equal the logits of its chunks bit for bit at EVERY chunk size (default: above that size)
 *   attn_window        1               0 = block 0's attention backward on all rows instead of the prompt rows' blocks
 *   last_single        1 (0 exact)     0 = the last block's attention on all rows instead of the single-query form
 *   attn_two_kernels   0               1 = attention backward as the dQ + dK/dV kernel pair
 *   attn_fused_w1      0               1 = fused attention backward with two 16-row blocks per wave
 *   lp_grad            fp16: 0, else 1 gradient stream of the residual in T (bf16 mode: 0 also returns the forward's update stream to fp32;
 *                                      fp16 mode: 1 trades 30 % more gradient error for 0.9 ms)
 *   lp_upd             bf16: 1, else 0 the forward's update stream in T (fp16 mode: would cost 2e-4 of logit error)
 *   gelu_q8            bf16: 1, else 0 c_fc keeps QuickGELU'(u) in 8 bits for the backward instead of u in T (2.4e-3 on a factor in [-0.1, 1.1]:
 *                                      bf16's own grade; towers without split operands).  Between steps only: the backward decodes what the
 *                                      forward stored
 *   txt_split          fp16 / fp32: 1  0 = no split operands in the text tower (fp16 mode; only before the first mudpt_set_weight)
 *   txt_lo             fp16 / fp32: 1  form of the text tower's low halves: 0 = none, 1 = fp16 pairs (txt_split is its older name)  } MUDPT_F32 above
 *   vis_lo             fp32: 2, else 0 ... of the vision tower's: 2 = e4m3 remainders on the fp8 matrix pipe (parity mode only)         } and DESIGN.md 2;
 *   vis_sites          31              bit mask of the sites that split: 1 in_proj, 2 out_proj, 4 c_fc, 8 c_proj, 16 patch embed       } effective from
 *   txt_sites          31              ... of the text tower                                                                           } the next forward
 *   vis_exact_attn     0               1 = the vision tower's attention forward in fp32 (parity mode only)                             }
 *   txt_exact_attn     fp32: 1, else 0 ... the text tower's (parity mode only)                                                         }
 *   txt_trim           1               0 = run the text tower on all ctx_len positions        } read by the next
 *   txt_buckets        3               maximum number of length buckets of the class prompts  } mudpt_set_class_prompts,
 *   txt_bucket_cost    1024            token rows one more bucket must save                   } which must follow
 *   cocoop_chunk       0 (= budget)    cap on the images per CoCoOp text-tower pass           }
 *   prof_stride        1               measurement mode brackets every prof_stride-th persistent-GEMM launch, counted across steps */
int mudpt_model_set(mudpt_model* m, const char* name, int32_t value);

/* Measurement hook (bench.py): bracket every MFMA GEMM launch of the path with HIP events on its launch stream.
 * mudpt_profile_read synchronises and returns the summed duration, the summed algorithmic FLOPs (2 M N K) and
 * the number of launches since the last enable / read. */
/* enable: 0 = off; 1 = the persistent MFMA GEMM launches only (class 0 below); otherwise a bit mask of the classes of
 * mudpt_profile_read_classes (31 = all).  An event pair costs ~5 us of queue time per bracketed launch (measured: 157 pairs = 0.8 ms
 * per step), so the timed region of bench.py brackets the dominant kernel only and the other classes are measured in a separate pass. */
int mudpt_profile_enable(mudpt_model* m, int32_t enable);
int mudpt_profile_read(mudpt_model* m, double* gemm_ms, double* gemm_flop, int64_t* launches);
/* The same per kernel class (arrays of MUDPT_PROF_CLASSES entries): 0 the persistent MFMA GEMM (work = algorithmic FLOPs), 1 / 2
 * LayerNorm forward / backward, 3 / 4 attention forward / backward (dQ + dK/dV kernels together) of the vision tower (work =
 * algorithmic HBM bytes: every operand read once, every result written once).  executed_flop (may be NULL): MFMA FLOPs actually
 * executed by all GEMM and attention launches of both towers. */
#define MUDPT_PROF_CLASSES 5
int mudpt_profile_read_classes(mudpt_model* m, double* ms, double* work, int64_t* launches, double* executed_flop);

/* ---- the input pipeline on the device (stateless: no model handle; additions, so MUDPT_ABI_VERSION stays) ---------------------------
 * What they replace: Dassl's training transform of every shipped yaml -- INPUT.TRANSFORMS ("random_resized_crop", "random_flip",
 * "normalize") with INTERPOLATION "bicubic", run per image and step in Pillow on the loader's CPU workers (torchvision RandomResizedCrop's
 * F.resized_crop = img.crop(box).resize((S, S), BICUBIC), hflip, ToTensor, Normalize) -- and the [B, 3, S, S] fp32 host -> device copy of
 * parse_batch_train (trainers/mudpt.py:263-268).  Images are decoded ONCE into a flat uint8 HWC store in device memory; per step the host
 * draws a few integers per sample and one launch writes the batch mudpt_forward_backward takes.  The evaluation transform
 * (Resize(S) on the short side + CenterCrop(S)) is an instance of the same operation.
 *
 * params row n = (image, flip, x_lo, x_len, x_out, x_off, y_lo, y_len, y_out, y_off), int32.  Per axis (in_len, out_len, out_off, lo from
 * the row; o in [0, size)), all in fp64, Pillow's ImagingResample rule by rule:
 *   scale = in_len / out_len; fs = max(scale, 1); support = 2 fs; center = (o + out_off + 0.5) scale;
 *   taps t in [max(0, (int)(center - support + 0.5)), min(in_len, (int)(center + support + 0.5)));
 *   raw weight f((t - center + 0.5) / fs), f the cubic with a = -0.5; divided by their sum (added in ascending t);
 *   fixed point k_t = (int)(w 2^22 + (w < 0 ? -0.5 : 0.5)); tap t reads source index lo + t;
 *   a pass: acc = 2^21 + sum k_t byte_t in int32, result byte = clamp(acc >> 22, 0, 255).
 * The horizontal pass runs first and is rounded to bytes, the vertical pass runs on those bytes; flip writes column size - 1 - o; byte b of
 * channel c becomes (float(b) / 255.0f - mean[c]) / std[c] in IEEE fp32 (ToTensor + Normalize); out[n, c, y, x] planar.
 *   training  (crop box i, j, h, w):  x_lo = j, x_len = w, x_out = size, x_off = 0; y likewise with i, h
 *   evaluation: x_lo = 0, x_len = W, x_out = Wr, x_off = round((Wr - size) / 2), Wr = size on the short side, int(size long / short) on the other
 * (Pillow 12.2.0 itself was seen to run vertical-then-horizontal on sources 8 pixels wide and >= 900 rows high; this library never does.)
 *
 * mudpt_augment: pixels_dev the store; images_dev [n_images, 3] = byte offset, height, width of each image; params_dev [batch, 10];
 * mean_std_host six HOST floats (mean[3], std[3]), read before the call returns; out_dev [batch, 3, size, size] fp32.  Asynchronous on `stream`.
 * MUDPT_ERR_ARG before any GPU call: a null pointer, batch < 0, size < 1; batch == 0 launches nothing.  The kernel TRUSTS both tables. */
int mudpt_augment(const uint8_t* pixels_dev, const int64_t* images_dev, int32_t n_images, const int32_t* params_dev, int32_t batch, int32_t size,
                  const float* mean_std_host, float* out_dev, void* stream);
/* HOST only: validates HOST copies of the two tables before they are uploaded.  images: heights and widths >= 1, offsets >= 0 and ascending
 * with room for 3 H W bytes each; params: image in [0, n_images), flip 0 | 1, x_len / x_out / y_len / y_out >= 1, lo >= 0 and lo + len
 * inside the image, out_off >= 0 and out_off + size <= out_len.  MUDPT_ERR_ARG with a message that names the table, the row and the column. */
int mudpt_augment_check(const int64_t* images_host, int32_t n_images, const int32_t* params_host, int32_t batch, int32_t size);
/* HOST arithmetic only: the kernel form one sample takes (every form writes the same bytes), as form | R << 8; -1 for a length < 1.
 * TABLE while the tables and R rows' worth of source rows fit the workgroup's 40 000 bytes of LDS, for the largest R of 16, 8, 4, 2, 1:
 *   3072 + 8 size + 4 size kx + 128 + 64 ky + rows(R) 3 ceil4(size),  kx / ky = 2 ceil(support) + 1,
 *   rows(R) = (int)((R - 1) scale_y + 2 support_y + 1) + 2;   DIRECT otherwise (R = 0). */
#define MUDPT_AUGMENT_TABLE 0  /* augment_kernel: weight tables and the horizontal pass in LDS, 16-byte stores */
#define MUDPT_AUGMENT_DIRECT 1 /* the same kernel, a thread per output pixel, every weight recomputed where it is used */
int mudpt_augment_form(int32_t x_len, int32_t x_out, int32_t y_len, int32_t y_out, int32_t size);

/* ---- single kernels, exported for parity tests (all pointers device memory) ---------------------------- */
/* epilogues: 0 store T | 1 bias+QuickGELU (out0 = u, out1 = gelu(u)) | 2 f32 out0 = aux + acc + bias |
 *            3 out0 = acc * QuickGELU'(aux) | 4 patch-embed scatter + pos | 5 store f32 */
int mudpt_gemm(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda,
               const void* B, int32_t ldb, const float* bias, void* out0, int32_t ldo0, void* out1, int32_t ldo1,
               const void* aux, int32_t ldaux, int32_t patches, int32_t seq_len, const float* pos, int32_t variant, void* stream);
/* variant: kernel-choice knob for tests / tuning (0 = the default dispatch).  Bit 16: allow split K.  Bit 17: QuickGELU' in 8 bits (what the
 * bf16 mode keeps for the backward instead of u): epilogue 1 writes out0 = byte codes rint((QuickGELU'(u) + 0.1) * 212) with a row stride of
 * ldo0 BYTES, epilogue 3 reads such codes from aux (row stride ldaux bytes). */
/* HOST arithmetic only: the kernel mudpt_gemm / mudpt_gemm_split runs for these arguments on a device of ncu compute units, as
 * form | slices << 8 (slices = 1 except for the split-K forms); -1 for arguments the launcher refuses (the checks that read no pointer:
 * shape, ldo0 / ldo1 / ldaux, epilogue, lo_mode).  variant as in mudpt_gemm: the low byte is the knob, bit 16 = scratch for split K is
 * available; the other bits do not change the form.  The first rule that matches (mudpt_amd/csrc/gemm.hip gemm_form):
 *   1. PP: knob 0 | 3 | 5 | 6 | 12, epilogue 0 | 1 | 3 | 5, at least 128 tiles of 256 x 256 (knob 3: 256), ldo0 % 8 == 0 (epilogue 1: ldo1, 3: ldaux too)
 *   2. SPLITK_K128 / _K64: epilogue 0 | 5, scratch, knob 0 | 12, no split operand, K >= 1536, 2 * (64 x 64 tiles) <= 5 ncu, and 2 .. 4 slices fit
 *   3. M * N >= 256 * 128 * 512: T256x256; knob 2: T128x256; knob 4: T256x128
 *   4. T64x64_K128 / T64x64 on small grids (knob 0; 12: never K128) or under knob 10 / 9;  5. T128x64_RING4: knob 6, or at most 128 tiles of
 *      128 x 128 and not knob 5;  6. T128x128. */
#define MUDPT_GEMM_PP 0            /* gemm_pp_kernel: persistent 256 x 256 ping-pong tiles */
#define MUDPT_GEMM_T256x256 1      /* gemm_nt_kernel 256 x 256 x 64, 8 waves */
#define MUDPT_GEMM_T128x256 2      /* gemm_nt_kernel 128 x 256 x 64, 8 waves */
#define MUDPT_GEMM_T256x128 3      /* gemm_nt_kernel 256 x 128 x 64, 8 waves */
#define MUDPT_GEMM_T64x64_K128 4   /* gemm_nt_kernel 64 x 64 x 128, 4 waves */
#define MUDPT_GEMM_T64x64 5        /* gemm_nt_kernel 64 x 64 x 64, 4 waves */
#define MUDPT_GEMM_T128x64_RING4 6 /* gemm_nt_kernel 128 x 64 x 64, 4 waves, 4-deep operand ring */
#define MUDPT_GEMM_T128x128 7      /* gemm_nt_kernel 128 x 128 x 64, 4 waves */
#define MUDPT_GEMM_SPLITK_K128 8   /* K slices of the 64 x 64 x 128 kernel + splitk_reduce_kernel */
#define MUDPT_GEMM_SPLITK_K64 9    /* K slices of the 64 x 64 x 64 kernel + splitk_reduce_kernel */
int mudpt_gemm_form(int32_t epilogue, int32_t M, int32_t N, int32_t K, int32_t ldo0, int32_t ldo1, int32_t ldaux, int32_t lo_mode, int32_t variant,
                    int32_t ncu);
/* A GEMM with a SPLIT A operand (the forward GEMMs of the parity mode): A = T(v), A_lo = the remainder v - A in a second buffer
 * with the row stride of A in bytes.  lo_mode 1: A_lo holds T values and a second pass contracts it against the same B (22 bits); lo_mode 2:
 * A_lo holds OCP e4m3 bytes of (v - A) * 2^12 (the first K bytes of each row) and the second pass runs on the MX-scaled fp8 matrix
 * instruction against B8, the e4m3 copy of B ([N, K] bytes at the row stride of B in bytes, values B * 2^shift, b8_scale = 127 - shift =
 * the E8M0 block scale); K % 128 == 0 and dtype fp16 then.  lo_mode 0: no second pass.  epilogue 0 | 1 | 2 | 3 | 5 as mudpt_gemm (4 needs
 * mudpt_gemm_split_patch's operands; the persistent kernel builds the e4m3 second pass for 0 | 1 | 5 only and refuses 3 at its sizes); with
 * epilogue 1, out1_lo (may be NULL) receives the low half of out1 = QuickGELU(u) in form out1_lo_mode (1 / 2), at the row stride of out1 in bytes. */
int mudpt_gemm_split(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, const void* A, const void* A_lo, int32_t lo_mode, int32_t lda,
                     const void* B, const void* B8, int32_t b8_scale, int32_t ldb, const float* bias, void* out0, int32_t ldo0, void* out1,
                     void* out1_lo, int32_t out1_lo_mode, int32_t ldo1, const void* aux, int32_t ldaux, int32_t variant, void* stream);
/* HOST helper (no device work): out[i] = OCP e4m3 (round to nearest even, saturating at +-448) of in[i] * 2^shift -- the conversion the
 * library applies to the frozen weights for the e4m3 second pass. */
int mudpt_e4m3_from_f32(const float* in_host, uint8_t* out_host, size_t n, int32_t shift);
/* LayerNorm forward writing a split operand: out = T(y), out_lo = the remainder in form lo_mode (1: T, 2: e4m3 bytes of (y - out) * 2^12),
 * rows of ldo elements of T / 2 ldo bytes. */
int mudpt_layernorm_fwd_split(int32_t dtype, const float* x, int32_t ldx, const float* gamma, const float* beta, void* out, void* out_lo,
                              int32_t lo_mode, int32_t ldo, int32_t rows, int32_t d, void* stream);
int mudpt_layernorm_fwd(int32_t dtype, const float* x, int32_t ldx, const int32_t* row_index, const float* gamma,
                        const float* beta, void* out, int32_t ldo, int32_t out_f32, float* mean, float* rstd,
                        int32_t rows, int32_t d, void* stream);
int mudpt_layernorm_bwd(int32_t dtype, const void* dy, int32_t lddy, int32_t dy_f32, const float* x, int32_t ldx,
                        const int32_t* row_index, const float* mean, const float* rstd, const float* gamma,
                        const float* dres, int32_t lddres, float* dx, int32_t lddx, void* dx_lp, int32_t lddx_lp,
                        int32_t rows, int32_t d, void* stream);
int mudpt_attention_padded_len(int32_t L);
/* causal: bit 0 = causal mask; bit 1 (tests / A-B, 224 < L <= 640 only) = the staged 16-query-block kernel instead of the resident one. */
int mudpt_attention_fwd(int32_t dtype, const void* qkv, void* out, float* lse, int32_t B, int32_t L, int32_t H,
                        int32_t causal, void* stream);
/* The fp32 attention forward (parity mode MUDPT_F32: the text tower, knob for the vision tower): q | k | v in fp32 [B, L, 3*H*64] -> the
 * output as a split operand out_hi (fp16) + out_lo (may be NULL; form lo_mode 1 / 2 as in mudpt_gemm_split; row stride ld_out elements of
 * fp16 = 2 ld_out bytes, 0 = H*64), lse, and -- if qkv_lp is not NULL -- the fp16 copy of q | k | v the backward kernels read. */
int mudpt_attention_fwd_exact(const float* qkv32, void* qkv_lp, void* out_hi, void* out_lo, int32_t lo_mode, int32_t ld_out, float* lse, int32_t B,
                              int32_t L, int32_t H, int32_t causal, void* stream);
/* causal: bit 0 = causal mask; the other bits choose among kernels that compute the same gradients (tests / A-B): bit 1 = two kernels, bit 3 =
 * force the fused pass, bit 2 = the same with two 16-row blocks per wave, bit 4 = sweep, bits 20-27 = n > 0: the window form on the n rows
 * per sequence from row bits 8-19 on (block 0 of a tower needs its input gradient on the prompt rows only: the 16-row blocks -- L > 224:
 * 128-row groups -- that hold a wanted row are computed exactly as without the window, all other rows of dqkv are left unwritten).
 * Which form runs (mudpt_attention_form names it; the kernels behind each: mudpt_amd/csrc/attention.hip):
 *   L <= 224, the first rule that matches:  1. one wanted row (mudpt_attention_bwd_sel), a window, or bit 1 -> TWO (dQ kernel + dK/dV kernel)
 *      2. bit 3 or 2 -> FUSED_W2, with bit 2 FUSED_W1 (bit 4 loses)   3. non-causal and (L >= 97 or bit 4) -> SWEEP (the vision tower)
 *      4. L <= 96 -> FUSED_W2 (the text tower; FUSED_W1 under the model knob attn_fused_w1)   5. causal, 97 .. 224 -> TWO
 *   L > 224:  L <= 608 (both operands of a (sequence, head) pair fit LDS) and none of rule 1 -> RESIDENT, else STAGED; bits 2 - 4 are ignored. */
int mudpt_attention_bwd(int32_t dtype, const void* qkv, const void* out, const void* dout, const float* lse,
                        float* delta, void* dqkv, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream);
/* HOST arithmetic only: the form mudpt_attention_fwd (bwd = 0; L <= 224: PAIR if causal, else PERSISTENT, bit 1 ignored; 225 .. 640: RESIDENT,
 * with bit 1 STAGED; beyond: STAGED) or mudpt_attention_bwd (bwd != 0; sel != 0: mudpt_attention_bwd_sel) runs for sequence length L and the
 * `causal` argument `flags`.  -1 for L outside 1 .. 4096. */
#define MUDPT_ATTN_FWD_PAIR 0       /* attn_fwd_pair_kernel: one workgroup per pair */
#define MUDPT_ATTN_FWD_PERSISTENT 1 /* attn_fwd_kernel: resident workgroups walk the pairs */
#define MUDPT_ATTN_FWD_RESIDENT 2   /* attn_fwd_resident_kernel: K and V of a pair in one CU's whole LDS */
#define MUDPT_ATTN_FWD_STAGED 3     /* attn_fwd_tiled_kernel: K and V stream through 64-row stages */
#define MUDPT_ATTN_BWD_TWO 4        /* attn_bwd_dq_kernel + attn_bwd_dkv_kernel */
#define MUDPT_ATTN_BWD_FUSED_W2 5   /* attn_bwd_fused_kernel, one 16-row block per wave */
#define MUDPT_ATTN_BWD_FUSED_W1 6   /* attn_bwd_fused_kernel, two 16-row blocks per wave */
#define MUDPT_ATTN_BWD_SWEEP 7      /* attn_bwd_sweep_kernel */
#define MUDPT_ATTN_BWD_RESIDENT 8   /* attn_bwd_dq_resident_kernel + attn_bwd_dkv_resident_kernel */
#define MUDPT_ATTN_BWD_STAGED 9     /* attn_bwd_dq_tiled_kernel + attn_bwd_dkv_tiled_kernel */
int mudpt_attention_form(int32_t bwd, int32_t L, int32_t flags, int32_t sel);
/* Single-query attention of a tower's LAST block (only the CLS / EOT row of its output is used, clip/model.py:549, trainers/mudpt.py:154):
 * one query per sequence -- q_sel [B, H*64], the query of token row sel_rows[b] (= b * L + position) -- against the K / V thirds of the
 * packed qkv buffer (causal: keys 0 .. position).  Forward: out_sel [B, H*64], lse_sel [B, H].  Backward: dq_sel [B, H*64] and the k, v
 * thirds of dqkv for EVERY row (zeros behind a causal limit); the q third of dqkv is not written. */
int mudpt_attention_fwd_single(int32_t dtype, const void* qkv, const void* q_sel, const int32_t* sel_rows, void* out_sel, float* lse_sel,
                               int32_t B, int32_t L, int32_t H, int32_t causal, void* stream);
int mudpt_attention_bwd_single(int32_t dtype, const void* qkv, const void* q_sel, const int32_t* sel_rows, const void* out_sel,
                               const void* dout_sel, const float* lse_sel, void* dqkv, void* dq_sel, int32_t B, int32_t L, int32_t H,
                               int32_t causal, void* stream);
/* LayerNorm forward with everything the transformer block fuses into it (clip/model.py:281-301): v = x[r] + add[r] (fp32 add or T
 * add_lp, either may be NULL; row stride ldadd); rows whose position (r % ov_L) lies in [ov_row0, ov_row0 + ov_n) are REPLACED by
 * ov_rows[(r % ov_L) - ov_row0] (the deep-prompt splice); v is written to xout (fp32, may be NULL) and normalised into out (T or fp32). */
int mudpt_layernorm_fwd_fused(int32_t dtype, const float* x, int32_t ldx, const float* add, const void* add_lp, int32_t ldadd,
                              const float* ov_rows, int32_t ov_row0, int32_t ov_n, int32_t ov_L, float* xout, int32_t ldxout,
                              const float* gamma, const float* beta, void* out, int32_t ldo, int32_t out_f32, float* mean,
                              float* rstd, int32_t rows, int32_t d, void* stream);
/* Cosine-logit head + mean cross-entropy, forward and backward (trainers/mudpt.py:178-182,250): logits[B, C] = scale *
 * normalise(img) . normalise(txt)^T, loss[0] = mean CE, dimg / dtxt = gradients of (grad_scale * loss) w.r.t. the RAW features.
 * labels / loss / dimg / dtxt may be NULL (forward only).  Scratch is allocated and freed inside (synchronises: a test hook). */
int mudpt_head(const float* img, const float* txt, const int64_t* labels, float scale, float grad_scale, int32_t B, int32_t C,
               int32_t e, float* logits, float* loss, float* dimg, float* dtxt, void* stream);
/* out[i, :] (+)= scale * sum_b src[b, row0 + i, :], b ascending in a fixed tree (bitwise reproducible): the backward of the prompt
 * splice.  src_f32 [B, L, d] or its T copy src_lp (at least one non-NULL); zero_src clears the summed rows afterwards. */
int mudpt_reduce_rows(int32_t dtype, float* src_f32, void* src_lp, int32_t B, int32_t L, int32_t d, int32_t row0, int32_t n,
                      float* out, int32_t zero_src, int32_t accumulate, float scale, void* stream);
/* CoCoOp (trainers/cocoop.py:141-146,187-194): dbias[i, :] = scale * sum over image i's C prompts and their n context rows (rows
 * 1..n of every L-row sequence) of the text-input gradient dx [B * C, L, d] (fp32, or its T copy dx_lp); fixed order: reproducible. */
int mudpt_cocoop_dbias(int32_t dtype, const float* dx_f32, const void* dx_lp, float* dbias, int32_t B, int32_t C, int32_t L, int32_t d,
                       int32_t n, float scale, void* stream);
/* CoOp (trainers/coop.py): the gradient of the context from the text-input gradient dx (fp32, or its T copy dx_lp).  rows [C * n]: token row
 * of context row j of class c.  csc = 0: dctx[j, :] = scale * sum_c dx[rows[c n + j], :] in a fixed order (reproducible bit for bit);
 * csc = 1: dctx[c, j, :] = scale * dx[rows[c n + j], :].  d % 64 == 0. */
int mudpt_coop_dctx(int32_t dtype, const float* dx_f32, const void* dx_lp, const int32_t* rows, float* dctx, int32_t C, int32_t n, int32_t d,
                    int32_t csc, float scale, void* stream);
/* fp32 C[M,N] = alpha * op(A) . op(B) (+ bias[N]) (+ beta * C): the prompt projections (trainers/mudpt.py:127-128, clip/model.py:539). */
int mudpt_sgemm(int32_t transA, int32_t transB, int32_t M, int32_t N, int32_t K, float alpha, const float* A, int32_t lda,
                const float* B, int32_t ldb, float beta, float* C, int32_t ldc, const float* bias, void* stream);
/* mudpt_optim_step without a handle: one update of p [n] from g [n] with the state slots of `optim`, every check of mudpt_optim_step's launcher
 * (they read no device memory, so they answer without a GPU). */
int mudpt_optim_apply(const mudpt_optim* optim, float* p, const float* g, int64_t n, void* stream);

/* ---- the launchers' production forms (test surface like the rest of this section: additions here leave MUDPT_ABI_VERSION alone, it
 * numbers the drop-in boundary above the line) ---- */
/* mudpt_layernorm_bwd plus what the training step passes: the residual gradient in T (dres_lp, same stride lddres; exclusive with dres),
 * the fused splice backward -- rows whose position r % side_L lies in [side_row0, side_row0 + side_n) go, in fp32, to
 * side[(r / side_L) * side_ldb + (pos - side_row0) * d] and ZERO goes to dx / dx_lp (identity row map only; side = NULL: off) -- and the
 * index mode of a row_index launch: 0 dy / mean / rstd compact (row r), 1 all three by token row (row_index[r]), 2 mean / rstd by token row. */
int mudpt_layernorm_bwd_ex(int32_t dtype, const void* dy, int32_t lddy, int32_t dy_f32, const float* x, int32_t ldx, const int32_t* row_index,
                           const float* mean, const float* rstd, const float* gamma, const float* dres, const void* dres_lp, int32_t lddres,
                           float* dx, int32_t lddx, void* dx_lp, int32_t lddx_lp, float* side, int32_t side_row0, int32_t side_n, int32_t side_L,
                           size_t side_ldb, int32_t index_mode, int32_t rows, int32_t d, void* stream);
/* mudpt_layernorm_fwd_fused with the launcher's remaining operands: a row map (row_index, as mudpt_layernorm_fwd: only WITHOUT add / splice /
 * xout, which the launcher refuses under a row map) and a split output (out_lo in lo_mode 1 / 2, as mudpt_layernorm_fwd_split: T output only). */
int mudpt_layernorm_fwd_ex(int32_t dtype, const float* x, int32_t ldx, const int32_t* row_index, const float* add, const void* add_lp, int32_t ldadd,
                           const float* ov_rows, int32_t ov_row0, int32_t ov_n, int32_t ov_L, float* xout, int32_t ldxout, const float* gamma,
                           const float* beta, void* out, void* out_lo, int32_t lo_mode, int32_t ldo, int32_t out_f32, float* mean, float* rstd,
                           int32_t rows, int32_t d, void* stream);
/* mudpt_attention_fwd / _fwd_single writing a split output (the parity mode's vision tower): out = T(O) in rows of ld_out elements (0 = H*64),
 * out_lo (may be NULL) = the remainder in form lo_mode (1: T; 2: e4m3 bytes of (O - out) * 2^12, the first H*64 bytes of each row) at the same
 * row stride in bytes. */
int mudpt_attention_fwd_split(int32_t dtype, const void* qkv, void* out, void* out_lo, int32_t lo_mode, int32_t ld_out, float* lse, int32_t B, int32_t L,
                              int32_t H, int32_t causal, void* stream);
int mudpt_attention_fwd_single_split(int32_t dtype, const void* qkv, const void* q_sel, const int32_t* sel_rows, void* out_sel, void* out_lo,
                                     int32_t lo_mode, int32_t ld_out, float* lse_sel, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream);
/* mudpt_attention_bwd where dout is zero except on token row sel_rows[b] (= b * L + position) of every sequence (the last block with the
 * knob last_single = 0, the class-parallel path): query blocks without that row are skipped.  causal: bit 0 only. */
int mudpt_attention_bwd_sel(int32_t dtype, const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                            const int32_t* sel_rows, int32_t B, int32_t L, int32_t H, int32_t causal, void* stream);
/* mudpt_head with the state the model keeps between calls in the caller's hands: txt_n [C, e] / txt_inv [C] (txt = NULL: reuse them as the
 * previous call left them -- the fused path only), B_total > 0 (this call is a chunk of a batch of B_total images: gradients are scaled by
 * 1 / B_total and `loss` is NOT written, the caller takes the mean of the row losses), row_loss [B] (may be NULL).  path 0: the dispatch of
 * mudpt_head; 1: force the unfused launchers.  *path_taken (HOST, may be NULL) = 0 if the fused kernels ran, 1 if the unfused ones.
 * Training (labels given) needs `loss`; dimg may be NULL: no image gradient is computed (the head of a frozen, prompt-free image tower, as
 * on a mudpt_create_resnet handle).  Every other output is then bit-identical to the call with dimg.  The fused training kernels take a
 * shape if e % 16 == 0, e <= 1024 and ((dimg ? 32 : 16) e + 16 roundup(C, 16)) 4 + 256 <= 163840 bytes of LDS: without dimg that is the
 * forward's rule plus e <= 1024 (e = 1024: C <= 1520 instead of 496; e = 512: C <= 2032 instead of 1520). */
int mudpt_head_ex(const float* img, const float* txt, const int64_t* labels, float scale, float grad_scale, int32_t B, int32_t B_total, int32_t C,
                  int32_t e, float* txt_n, float* txt_inv, float* logits, float* loss, float* row_loss, float* dimg, float* dtxt, int32_t path,
                  int32_t* path_taken, void* stream);
/* The head's backward from a GIVEN logit gradient, on the state a head forward left (img_n [B, e] / img_inv [B] / txt_n [C, e] / txt_inv [C]; the
 * caller owns every buffer; asynchronous on `stream`):
 *   dimg = gmul * (l2norm_bwd(scale * G   . txt_n, img_n, img_inv) + Eimg)   [B, e]     l2norm_bwd(d, n, inv) = inv * (d - n <d, n>) per row
 *   dtxt = gmul * (l2norm_bwd(scale * G^T . img_n, txt_n, txt_inv) + Etxt)   [C, e]
 * G [B, C] fp32 at row stride ldg >= C (the padding columns are never read), Eimg, Etxt: each may be NULL, not all three; dimg / dtxt: either may
 * be NULL (not computed), not both.  G NULL: no contraction, the outputs are gmul * E bit for bit (zeros where that E is NULL).  The contraction
 * runs in exact fp32 on the matrix cores in a fixed order; gmul is folded into its scale.  path 0, the dispatch: fused (one workgroup per 16
 * images resp. 16 classes, a [16][e] tile in LDS) if e % 16 == 0, e <= 1024, B <= 16 and C <= 16 (one workgroup per kernel: where it is the faster form), else unfused; 1: force
 * the unfused form (mudpt_sgemm twice + a row-wise kernel); 2: force the fused form (MUDPT_ERR_ARG where e does not fit).  *path_taken (HOST, may
 * be NULL) = 0 fused, 1 unfused; a refused call does not write it.  MUDPT_ERR_ARG before any launch, naming the field: a null state pointer, B, C or e < 1,
 * ldg < C, dimg and dtxt both NULL, G, Eimg and Etxt all NULL. */
int mudpt_head_grad(const float* img_n, const float* img_inv, const float* txt_n, const float* txt_inv, const float* G, int64_t ldg, const float* Eimg,
                    const float* Etxt, float scale, float gmul, int32_t B, int32_t C, int32_t e, float* dimg, float* dtxt, int32_t path,
                    int32_t* path_taken, void* stream);
/* CoCoOp's head (trainers/cocoop.py:187-197): every image has its own text features txt [B * C, e] (row i * C + c); logits[i, c] = scale *
 * <normalise(img_i), normalise(txt_{i,c})>, row_loss [B], dtxt [B * C, e] = gradient of (grad_scale * mean CE) w.r.t. the raw text features.
 * B_total > 0: a chunk of a batch of B_total images (gradients scaled by 1 / B_total, `loss` not written); 0: loss[0] = mean(row_loss).
 * labels NULL: logits only. */
int mudpt_pair_head(const float* img, const float* txt, const int64_t* labels, float scale, float grad_scale, int32_t B, int32_t B_total, int32_t C,
                    int32_t e, float* logits, float* loss, float* row_loss, float* dtxt, void* stream);
/* mudpt_gemm_split with the patch-embed epilogue's operands (epilogue 4 of mudpt_gemm: patches, seq_len, pos): what the parity mode's vision
 * tower runs on the split patch rows mudpt_patchify writes.  Every other epilogue as mudpt_gemm_split. */
int mudpt_gemm_split_patch(int32_t dtype, int32_t epilogue, int32_t M, int32_t N, int32_t K, const void* A, const void* A_lo, int32_t lo_mode, int32_t lda,
                           const void* B, const void* B8, int32_t b8_scale, int32_t ldb, const float* bias, void* out0, int32_t ldo0, void* out1,
                           void* out1_lo, int32_t out1_lo_mode, int32_t ldo1, const void* aux, int32_t ldaux, int32_t patches, int32_t seq_len,
                           const float* pos, int32_t variant, void* stream);
/* images fp32 [B, 3, S, S] -> patches T [B * (S/p)^2, ldk], inner order (c, py, px), columns 3 p p .. ldk zero (clip/model.py:527-529);
 * patches_lo not NULL: the split form, the remainder in form lo_mode (1 / 2) in rows of 2 ldk bytes. */
int mudpt_patchify(int32_t dtype, const float* images, void* patches, void* patches_lo, int32_t lo_mode, int32_t B, int32_t image_size, int32_t patch,
                   int32_t ldk, void* stream);
/* The data movers, one launcher each (mudpt_amd/csrc/kernels.h has the definitions):
 *   set_rows        x[b, row0 + i, :] = rows[i, :] (+ add[i, :]), x fp32 [B, L, d]
 *   gather_rows     dst[r] = src[rows[r]]   } whole rows of row_bytes (a multiple of 16), strides in bytes
 *   scatter_rows    dst[rows[r]] = src[r]   }
 *   add_rows        dst[rows[r], :] += src[r, :] in T (one fp32 add, one rounding; rows distinct)
 *   colsum          out[n] (+)= sum_m A[m, n], A fp32 [M, N] with row stride lda
 *   add / cast      y = a + b (fp32) / y = T(x)
 *   relu / relu_bwd y = max(y, 0) in place / dy = y > 0 ? dy : 0 in place
 *   cocoop_prompts  x0[(i, c), l, :] = emb_pos[c, l, :], rows 1..n = ctx[l - 1] + bias[i] + pos[l]   (trainers/cocoop.py:148-165)
 *   coop_splice     x[rows[c n + j], :] = ctx[csc ? c : 0][j] + tpos[pos[c n + j]]                    (trainers/coop.py:99-164) */
int mudpt_set_rows(float* x, int32_t B, int32_t L, int32_t d, int32_t row0, int32_t n, const float* rows, const float* add, void* stream);
int mudpt_gather_rows(const void* src, size_t src_stride, const int32_t* rows, void* dst, size_t dst_stride, int32_t nrows, int32_t row_bytes, void* stream);
int mudpt_scatter_rows(const void* src, size_t src_stride, const int32_t* rows, void* dst, size_t dst_stride, int32_t nrows, int32_t row_bytes, void* stream);
int mudpt_add_rows(int32_t dtype, const void* src, const int32_t* rows, void* dst, int32_t nrows, int32_t d, void* stream);
/* Backward of one trained Linear y = x W^T + b in ONE launch (x [R, in], W [out, in], dy [R, out], dense fp32): dW = dy^T x, db = column sums of
 * dy, dx = dy W, all written; bit-identical to mudpt_sgemm(tA) + mudpt_colsum + mudpt_sgemm on the same operands.  Refused on the host: a null
 * pointer, a size < 1, dW / db / dx overlapping an input or each other. */
int mudpt_linear_bwd(int32_t R, int32_t out, int32_t in, const float* dy, const float* x, const float* W, float* dW, float* db, float* dx, void* stream);
int mudpt_colsum(const float* A, int32_t M, int32_t N, int32_t lda, float* out, int32_t accumulate, void* stream);
int mudpt_add(const float* a, const float* b, float* y, size_t n, void* stream);
int mudpt_cast(int32_t dtype, const float* x, void* y, size_t n, void* stream);
int mudpt_relu(float* y, size_t n, void* stream);
int mudpt_relu_bwd(float* dy, const float* y, size_t n, void* stream);
int mudpt_cocoop_prompts(float* x0, const float* emb_pos, const float* ctx, const float* bias, const float* pos, int32_t B, int32_t C, int32_t L,
                         int32_t d, int32_t n, void* stream);
int mudpt_coop_splice(float* x, const float* ctx, const float* tpos, const int32_t* rows, const int32_t* pos, int32_t C, int32_t n, int32_t d,
                      int32_t csc, void* stream);
/* Zero-shot CLIP's two kernels (mudpt_amd/csrc/zeroshot.hip).  Refused on the host: a null pointer, a size < 1, d (e) % 4 != 0.
 *   embed_tokens      out[r, :] = table[tokens_dev[r], :] + pos[positions_dev[r], :], r < rows, d fp32 per row, one add: bit-exact.  The ids
 *                     are DEVICE data the export cannot read: an id outside [0, vocab) -- or a position outside pos -- READS OUT OF BOUNDS;
 *                     checking them is the caller's job (mudpt_set_text_tokens checks its own on the host)
 *   feature_ensemble  one call per template in ascending order over f, acc, out [C, e] (three different tables): v = f / |f| per row; acc = v if
 *                     `first`, else acc + v; if `last`, out = normalise(acc / n_templates).  n_templates = 1 (first and last): out = v */
int mudpt_embed_tokens(const float* table, int32_t vocab, const int32_t* tokens_dev, const int32_t* positions_dev, const float* pos, float* out,
                       int32_t rows, int32_t d, void* stream);
int mudpt_feature_ensemble(const float* f, float* acc, float* out, int32_t C, int32_t e, int32_t first, int32_t last, int32_t n_templates, void* stream);
/* UMuDPT's prompt generator in fp32 (mudpt_amd/csrc/promptgen.hip), kernel by kernel:
 *   layernorm_bwd_affine  dx = (dres +) LN'(dy) and dgamma[j] (+)= sum_r dy[r, j] xhat[r, j], dbeta[j] (+)= sum_r dy[r, j] in row order (two runs
 *                         agree bit for bit); x / mean / rstd as mudpt_layernorm_fwd with out_f32 left them
 *   pg_attention_fwd      softmax(q k^T / 8) v on packed qkv [N, L, 3*H*64], 1 <= L <= 16, no mask; probs [N, H, L, L] saved for the backward
 *   pg_attention_bwd      dqkv [N, L, 3*H*64] from qkv, probs and dout [N, L, H*64];  d_model must equal H * 64
 *   quickgelu_fwd / _bwd  y = u sigmoid(1.702 u) / du = dy QuickGELU'(u) (du may be dy) */
int mudpt_layernorm_bwd_affine(const float* x, int32_t ldx, const float* mean, const float* rstd, const float* gamma, const float* dy, int32_t lddy,
                               const float* dres, int32_t lddres, float* dx, int32_t lddx, float* dgamma, float* dbeta, int32_t accumulate, int32_t rows,
                               int32_t d, void* stream);
int mudpt_pg_attention_fwd(const float* qkv, float* out, float* probs, int32_t N, int32_t L, int32_t H, int32_t d_model, void* stream);
int mudpt_pg_attention_bwd(const float* qkv, const float* probs, const float* dout, float* dqkv, int32_t N, int32_t L, int32_t H, int32_t d_model, void* stream);
int mudpt_quickgelu_fwd(const float* u, float* y, size_t n, void* stream);
int mudpt_quickgelu_bwd(const float* dy, const float* u, float* du, size_t n, void* stream);
/* The whole generator, the code the UMuDPT model path runs.  params: its 18 tensors in one flat fp32 buffer in the order of mudpt_param_info
 * (tensors 2 .. 19); X [depth * n_ctx, d_t] = cat(ctx, deep_prompts); G [depth * n_ctx, d_v].  workspace: fp32, at least
 * mudpt_promptgen_workspace(...) elements; the forward leaves there what the backward reads.  The backward WRITES grads (laid out as params)
 * and dX [depth * n_ctx, d_t].  Refused before any launch: depth < 1, n_ctx outside 1..16, d_t % 64 != 0, a short workspace. */
size_t mudpt_promptgen_workspace(int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v);
size_t mudpt_promptgen_param_numel(int32_t d_t, int32_t d_v);
int mudpt_promptgen_forward(int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v, const float* params, const float* X, float* G, float* workspace,
                            size_t workspace_numel, void* stream);
int mudpt_promptgen_backward(int32_t depth, int32_t n_ctx, int32_t d_t, int32_t d_v, const float* params, const float* X, const float* dG, float* dX,
                             float* grads, float* workspace, size_t workspace_numel, void* stream);
/* The linear probe's kernels (mudpt_amd/csrc/probe.hip; lpclip/linear_probe.py's LogisticRegression(solver="lbfgs")), exact fp32 on the matrix cores
 * (v_mfma_f32_32x32x2_f32), 128 x 128 x 32 tiles staged through LDS; any sizes >= 1 and any strides >= the row length.  Scalars travel as float.
 *   probe_gemm_nt     C [M, N] = A [M, K] . B [N, K]^T (+ bias[N], may be NULL): the logits Z = X W^T + b
 *   probe_gemm_tn     C [M, N] = A [Kd, M]^T . B [Kd, N] (+ beta W [M, N], may be NULL), db [M] (may be NULL) = column sums of A: dW = P^T X + beta W and
 *                     db = P^T 1 in one pass.  The depth is cut into slices of whole 32-deep steps (slices = 0: the library's choice for the device,
 *                     otherwise the wish, both as mudpt_probe_gemm_tn_slices reports), the partial sums go to scratch (slices * (M N + M) floats) and are
 *                     added in ascending order by a second kernel: no float atomics, two runs give the same bits.  C must not alias A, B or W.
 *   probe_gemm_tn_slices  HOST arithmetic only: the slice count for a wish (<= 0: two workgroups per compute unit of ncu, at least two steps a slice); -1 for sizes < 1
 *   probe_rows        Z [rows, n_cls] in place: logits -> P = (softmax - onehot(labels)) / rows; row_loss [rows] = logsumexp(z) - z[label] (computed as
 *                     log1p(sum of the other exponentials) + (max - z[label])); loss_sum[0] (a device double) = their sum in a fixed order.
 *                     labels int32 [rows] in [0, n_cls) are DEVICE data the kernel TRUSTS: the caller checks them on the host
 *   probe_argmax      pred[r] (int32) = the lowest index of the maximum of row r, as numpy.argmax; labels / count (both or neither, int32): count[0] = matches */
int mudpt_probe_gemm_nt(int32_t M, int32_t N, int32_t K, const float* A, int32_t lda, const float* B, int32_t ldb, const float* bias, float* C, int32_t ldc, void* stream);
int mudpt_probe_gemm_tn(int32_t M, int32_t N, int32_t Kd, const float* A, int32_t lda, const float* B, int32_t ldb, float beta, const float* W, int32_t ldw, float* C,
                        int32_t ldc, float* db, float* scratch, size_t scratch_numel, int32_t slices, void* stream);
int mudpt_probe_gemm_tn_slices(int32_t M, int32_t N, int32_t Kd, int32_t slices, int32_t ncu);
int mudpt_probe_rows(float* Z, int32_t ldz, const int32_t* labels, int32_t rows, int32_t n_cls, float* row_loss, double* loss_sum, void* stream);
int mudpt_probe_argmax(const float* Z, int32_t ldz, int32_t rows, int32_t n_cls, int32_t* pred, const int32_t* labels, int32_t* count, void* stream);
/* The test pass's evaluator (mudpt_amd/csrc/evaluate.hip; Dassl's Classification evaluator: accuracy, macro-F1, per-class results, confusion matrix).
 * Stateless additions without a model handle, so MUDPT_ABI_VERSION stays.  The state is ONE int32 device buffer of mudpt_eval_state_numel elements:
 *   [total, correct, invalid, reserved] [support: C] [predicted: C] [hit: C] [cmat: C x C, row = label, column = prediction; only when with_cmat]
 *   eval_state_numel  HOST arithmetic only: 4 + 3 C (+ C^2 with_cmat); 0 for n_cls < 1, or with_cmat and C^2 >= 2^31
 *   eval_reset        zeroes the state
 *   eval_accumulate   logits [rows, n_cls] fp32 (row stride ldz >= n_cls), labels [rows] int64, both DEVICE data.  The prediction p of a row is what
 *                     torch.max(logits, 1)[1] gives on the CPU for the same values: the lowest index of the maximum; the index of the first NaN if the
 *                     row holds one; +0 == -0; a row of -inf gives 0 (NOT probe_argmax's rule, which skips NaN).  Every logit is read once (16-byte
 *                     loads when the base is 16-byte aligned and ldz % 4 == 0).  A label y outside [0, n_cls) adds one to invalid and nothing else
 *                     (it never indexes anything); a valid row adds one to total, support[y], predicted[p], to correct and hit[y] when p == y, and
 *                     to cmat[y][p] when with_cmat.  Integer atomics only: two runs give the same bits.  pred (int32 [rows], may be NULL) receives
 *                     p, -1 for an invalid row.  Nothing is reset: consecutive launches on one stream add up.
 *   eval_finalize     one launch; results (6 DEVICE doubles) = total, correct, invalid, n_supported = classes with support > 0,
 *                     macro_f1 = 100 x mean over those classes of 2 hit / (support + predicted)  (sklearn's f1_score(average="macro",
 *                     labels=np.unique(y_true))), perclass_accuracy = mean over them of 100 x hit / support; double sums in a fixed order, zeros
 *                     (never NaN) for an empty state.  It reads the first 4 + 3 C elements only.
 * MUDPT_ERR_ARG before any GPU call, no output touched: a null pointer (pred excepted), rows < 1, n_cls < 1, ldz < n_cls, with_cmat and n_cls^2 >= 2^31. */
size_t mudpt_eval_state_numel(int32_t n_cls, int32_t with_cmat);
int mudpt_eval_reset(int32_t* state, int32_t n_cls, int32_t with_cmat, void* stream);
int mudpt_eval_accumulate(const float* logits, int32_t ldz, const int64_t* labels, int32_t rows, int32_t n_cls, int32_t* state, int32_t with_cmat, int32_t* pred,
                          void* stream);
int mudpt_eval_finalize(const int32_t* state, int32_t n_cls, double* results, void* stream);
/* Top-k on the device (mudpt_amd/csrc/topk.hip): ranked predictions, their softmax, and the rank of every label.  Stateless additions without a
 * model handle, so MUDPT_ABI_VERSION stays.  logits [rows, n_cls] fp32 at row stride ldz >= n_cls, DEVICE data; 16-byte loads when the base is
 * 16-byte aligned and ldz % 4 == 0, the same results either way.
 * THE ORDER.  Column a precedes column b of a row z iff, on the key (isnan(z), z, -index): z[a] is NaN and (z[b] is not NaN or a < b); or neither
 * is NaN and (z[a] > z[b] or (z[a] == z[b] and a < b)).  +0 == -0.  It is mudpt_eval_accumulate's prediction rule carried to every place and
 * equals torch.sort(z, 1, descending=True, stable=True) on the CPU (NOT torch.topk, which returns ties in no defined order).
 *   topk             index (int32 [rows, k]) = the first k columns of every row in that order; index[:, 0] is mudpt_eval_accumulate's pred.
 *                    value (fp32 [rows, k], may be NULL) = their logits bit for bit (a NaN's payload excepted).  prob (fp32 [rows, k], may be
 *                    NULL) = the softmax of the WHOLE row at those columns: m = the logit of the first column (the row maximum, or a NaN);
 *                    terms expf(z - m), the accurate expf; lane l of a 64-lane wave adds, in ascending column order, the terms of columns
 *                    4 l .. 4 l + 3 (+ 256, + 512, ..) below n_cls & ~3 and then of column (n_cls & ~3) + l; the 64 sums are added by an xor
 *                    tree (32, 16, .. 1); prob = expf(z - m) / sum, one division per output.  The chain is fixed: a row gives the same bits in
 *                    every run, at every position of every batch, at every ldz and alignment.  A row that holds a NaN, a +inf, or only -inf
 *                    gives NaN probabilities, as torch.softmax does.  No LDS, no sort: k rounds over the row, which a lane keeps in
 *                    registers up to n_cls = 1027; above that the first round reads memory and the others the cache.
 *   rank_accumulate  labels int64 [rows], DEVICE data.  The rank of a row's label y = the number of columns that precede y (0: y is
 *                    mudpt_eval_accumulate's prediction; it is the inverse permutation of the stable sort).  state: int32 [2 + kmax] =
 *                    [total, invalid, hist[0 .. kmax)], caller-owned and zeroed by the caller: a valid row adds one to total and, if its rank
 *                    is below kmax, to hist[rank]; a label outside [0, n_cls) adds one to invalid and nothing else (it never indexes
 *                    anything).  Top-k accuracy for any k <= kmax = sum(hist[:k]) / total.  Integer atomics only: two runs give the same
 *                    bits; nothing is reset: launches add up.  rank (int32 [rows], may be NULL) receives the full rank 0 .. n_cls - 1, -1 for
 *                    an invalid label.
 * MUDPT_ERR_ARG with a message that names the argument, before any GPU call, no output touched: a null logits, index, labels or state;
 * rows < 1; n_cls < 1; ldz < n_cls; k or kmax outside 1 .. 64; k > n_cls. */
int mudpt_topk(const float* logits, int32_t ldz, int32_t rows, int32_t n_cls, int32_t k, int32_t* index, float* value, float* prob, void* stream);
int mudpt_rank_accumulate(const float* logits, int32_t ldz, const int64_t* labels, int32_t rows, int32_t n_cls, int32_t kmax, int32_t* state, int32_t* rank,
                          void* stream);
/* The ResNet tower's memory movers (mudpt_amd/csrc/resnet.hip) and its host-side weight packing.  Activations are NHWC in T (dtype 0 bf16 / 1 fp16),
 * one pixel = one row of C channels (C % 8 == 0) at a row stride (elements) >= C that is a multiple of 8; every pointer 16-byte aligned.  Refused on
 * the host (MUDPT_ERR_ARG): a null pointer, a size < 1, a stride or alignment outside that.
 *   im2col           patch rows of a 3 x 3, pad 1 convolution of stride 1 | 2: dst [B * Ho * Wo, ldk] T, column (ky * 3 + kx) * C + c, Ho = (H - 1) / stride + 1,
 *                    ldk >= 9 C and ldk % 8 == 0; border taps and the columns from 9 C on are WRITTEN as zeros on every call.  src_planar != 0: src is
 *                    fp32 planar pixels [B, 3, H, W] (C must be 3, lds is not read), rounded to T
 *   bias_act         out [M, N] T = act(acc + bias + residual): acc fp32 (row stride ldacc, % 4 == 0), bias [N] fp32 or NULL, residual T or NULL,
 *                    relu != 0: max(., 0); both adds and the ReLU in fp32, ONE rounding.  N % 8 == 0
 *   avgpool2d        AvgPool2d(k): [B, H, W, C] -> [B, H / k, W / k, C]; the fp32 sum in window order (rows, then columns) times 1 / k^2, one rounding
 *   attnpool_tokens  AttentionPool2d's tokens (clip/model.py:76-78): [B, HW, C] -> [B, HW + 1, C]; row 0 = the fp32 mean over HW (sum in pixel order times
 *                    1 / HW), every row + pos [HW + 1, C] fp32, one rounding
 *   attnpool_attend  its attention for the pooled query (clip/model.py:79-97): q [B, H * 64] fp32 as q_proj left it (the kernel applies 64^-0.5), k / v rows
 *                    b * L + l of H * 64 fp32 at row stride ldkv, out [B, H * 64] T = softmax(q k^T / 8) v per head; fp32 throughout, one rounding
 *   conv_pack        HOST only, no device work: folds an eval-mode BatchNorm (eps 1e-5) into a bias-free convolution and packs it for the GEMM.  w
 *                    [cout, cin, k, k] (k = 1 | 3), gamma / beta / mean / var [cout]; in fp64 scale = gamma / sqrt(var + 1e-5), w' = w scale,
 *                    b' = beta - mean scale; w_out [cout, ldk] T (2-byte elements) = w' rounded ONCE from fp64, column (ky * k + kx) * cin + c, zeros from
 *                    k k cin on (ldk >= k k cin); bias_out [cout] fp32 = b' */
int mudpt_im2col(int32_t dtype, const void* src, int32_t src_planar, int32_t B, int32_t H, int32_t W, int32_t C, int32_t lds, int32_t stride, void* dst, int32_t ldk,
                 void* stream);
int mudpt_bias_act(int32_t dtype, const float* acc, int32_t ldacc, const float* bias, const void* residual, int32_t ldres, void* out, int32_t ldo, int32_t M, int32_t N,
                   int32_t relu, void* stream);
int mudpt_avgpool2d(int32_t dtype, const void* src, int32_t lds, void* dst, int32_t ldo, int32_t B, int32_t H, int32_t W, int32_t C, int32_t k, void* stream);
int mudpt_attnpool_tokens(int32_t dtype, const void* src, int32_t lds, const float* pos, void* dst, int32_t ldo, int32_t B, int32_t HW, int32_t C, void* stream);
int mudpt_attnpool_attend(int32_t dtype, const float* q, int32_t ldq, const float* k, const float* v, int32_t ldkv, void* out, int32_t ldo, int32_t B, int32_t L,
                          int32_t H, void* stream);
int mudpt_conv_pack(int32_t dtype, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, int32_t cout, int32_t cin, int32_t k,
                    int32_t ldk, void* w_out, float* bias_out);
/* The convolution as one kernel (mudpt_amd/csrc/conv.hip): an implicit GEMM that gathers the taps while it stages its operand, with bias, residual
 * and ReLU in its epilogue -- no patch rows and no fp32 accumulator go through memory.  An addition, so MUDPT_ABI_VERSION stays.
 *   out[b, oy, ox, n] = T(act(sum_{ky, kx, c} src[b, oy stride + ky - p, ox stride + kx - p, c] w[n, (ky k + kx) C + c] + bias[n] + residual[b, oy, ox, n]))
 *   k = 3: p = 1, stride 1 | 2;  k = 1: p = 0, stride 1.  Ho = (H - 1) / stride + 1, Wo likewise; a tap outside the image contributes zero.
 *   src       [B, H, W, C] T NHWC at channel stride lds: C % 8 == 0, lds >= C, lds % 8 == 0; channels C .. lds - 1 are never read
 *   w         [N, ldk] T as mudpt_conv_pack writes it: ldk >= k k C, ldk % 8 == 0; columns k k C .. ldk - 1 are never read.  N % 16 == 0
 *   bias      [N] fp32 or NULL;  residual [B Ho Wo, N] T at row stride ldres (>= N, % 4 == 0) or NULL (ldres is then not read)
 *   out       [B Ho Wo, N] T at row stride ldo (>= N, % 4 == 0); columns N .. ldo - 1 are not written
 *   The products are summed in fp32 on the 16-bit MFMA in column order, 32 columns per instruction; then + bias, + residual, ReLU (relu != 0)
 *   in fp32, in that order, and ONE rounding to T.  No split of K, no atomics, no workspace: a pixel's bits are the same in every run, at every
 *   position of every batch and in every tile form.
 * MUDPT_ERR_ARG before any launch, the message naming the argument: an unknown dtype; a null src, w or out; B, H, W, C or N < 1; k outside
 * {1, 3}; stride outside the above; C % 8; a bad lds, ldk, N, ldo or ldres; a pointer that is not 16-byte aligned; B H W beyond 31 bits.
 * mudpt_conv2d_form: HOST arithmetic only, the tile that runs M = B Ho Wo pixels x N channels (-1 for M or N < 1).  The first rule that matches,
 * counted in tiles against the MI355X's 256 compute units whatever the device: N > 64 and at least 256 tiles of 128 x 128: T128x128; at least
 * 256 tiles of 128 x 64: T128x64; T64x64. */
#define MUDPT_CONV_T128x128 0 /* conv2d_kernel, 128 pixels x 128 channels x 64, 4 waves */
#define MUDPT_CONV_T128x64 1  /* conv2d_kernel, 128 pixels x 64 channels x 64, 4 waves */
#define MUDPT_CONV_T64x64 2   /* conv2d_kernel, 64 pixels x 64 channels x 64, 4 waves */
int mudpt_conv2d(int32_t dtype, const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t lds, int32_t k, int32_t stride, const void* w, int32_t ldk,
                 const float* bias, const void* residual, int32_t ldres, void* out, int32_t ldo, int32_t N, int32_t relu, void* stream);
int mudpt_conv2d_form(int32_t M, int32_t N);
/* The text tower's sequence layout as mudpt_set_class_prompts / mudpt_set_text_tokens plan it, for eot [n_cls] (the EOT position of every class
 * prompt, 0 <= eot < ctx_len) and n_prompt prompt rows per sequence (0 <= n_prompt, n_prompt + 2 <= ctx_len).  HOST arithmetic only: no handle,
 * no device call; an addition, so MUDPT_ABI_VERSION stays.  txt_trim, txt_buckets, txt_bucket_cost: the knobs of mudpt_model_set; allow_buckets = 0
 * is CoCoOp's setting (always one bucket); heads >= 1 only spaces the buckets' LSE buffers.  The rule: a sequence keeps len = max(eot + 1,
 * n_prompt + 2) rows; untrimmed (txt_trim = 0) every sequence keeps ctx_len rows in one bucket.  One bucket runs every sequence to the longest
 * len, in the caller's order.  With allow_buckets, txt_trim, txt_buckets > 1 and n_cls x (longest len) >= 2048 the sequences are sorted by len
 * (a stable sort) and the sorted list is cut between distinct lengths into k <= txt_buckets buckets, each run to its longest member, so that
 * rows + k txt_bucket_cost is smallest; among the k of equal cost the smallest wins, and k = 1 keeps the caller's order.
 * Outputs, per packed sequence q (arrays of n_cls): cls[q] its class, first_row[q] its first packed row, bucket_len[q] the rows its bucket
 * runs it to; *buckets = k, *rows = the packed rows, *max_len = the longest kept length (what mudpt_text_layout reports for such a handle).
 * MUDPT_ERR_ARG with a message, nothing written: a null pointer, n_cls < 1, heads < 1, n_prompt or an eot outside the ranges above. */
int mudpt_text_layout_plan(const int32_t* eot, int32_t n_cls, int32_t ctx_len, int32_t n_prompt, int32_t heads, int32_t txt_trim, int32_t txt_buckets,
                           int32_t txt_bucket_cost, int32_t allow_buckets, int32_t* cls, int32_t* first_row, int32_t* bucket_len, int32_t* buckets, int32_t* rows,
                           int32_t* max_len);

#ifdef __cplusplus
}
#endif
#endif /* MUDPT_H */
