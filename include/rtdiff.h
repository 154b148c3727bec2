/* librtdiff — C ABI of the MI355X (gfx950) region-diffusion sampling engine.
 *
 * Drop-in boundary for the denoising hot path of songweige/rich-text-to-image.  The reference has no
 * native code and no FFI: its "operator interface" for this path is the Python call surface cited
 * beside each entry point below (file:line under /root/reference).  The Python facade in
 * rich-text-to-image_amd/ binds these symbols with ctypes and mirrors the reference classes.
 *
 * Conventions
 *   - every function returns int: 0 = ok, negative = RT_E_*; rt_last_error() gives the message
 *   - all tensor pointers are DEVICE pointers unless the parameter is documented as host
 *   - the caller owns every tensor it passes and keeps it alive until the stream is synchronised;
 *     the engine owns its weight arena, K/V caches, workspace and sampler state
 *   - one engine = one device = one HIP stream; calls on one engine are not re-entrant
 *   - no allocation happens inside forward / step calls
 */
#ifndef RTDIFF_H
#define RTDIFF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK 0
#define RT_E_INVALID (-1)
#define RT_E_HIP (-2)
#define RT_E_STATE (-3)
#define RT_E_MISSING_WEIGHT (-4)
#define RT_E_UNSUPPORTED (-5)

#define RT_MAX_LEVELS 4
#define RT_MAX_STREAMS 16

enum { RT_DTYPE_F32 = 0, RT_DTYPE_F16 = 1, RT_DTYPE_BF16 = 2 };
/* RT_SCHED_DPMPP_1 / _2: DPM-Solver++ (multistep, midpoint, epsilon prediction, lower-order final step) of order 1 / 2; either
 * UNet family, no input scaling, the x0 history of each stream kept in the engine */
enum { RT_SCHED_EULER = 0, RT_SCHED_PNDM = 1, RT_SCHED_DPMPP_1 = 2, RT_SCHED_DPMPP_2 = 3,
       /* stochastic samplers: a fresh N(0, 1) field per step, a pure function of (rt_set_noise_seed, step index, pixel), made on the device.
        * RT_SCHED_EULER_A: Euler ancestral, wherever RT_SCHED_EULER is accepted (sigma space, the same input scaling);
        * RT_SCHED_DPMPP_SDE_1 / _2: SDE-DPM-Solver++ of order 1 / 2, wherever the DPM-Solver++ kinds are (same history, same order rule) */
       RT_SCHED_EULER_A = 4, RT_SCHED_DPMPP_SDE_1 = 5, RT_SCHED_DPMPP_SDE_2 = 6 };

/* Architecture of the UNet: the constructor arguments of UNet2DConditionModel that SD-v1.5 / SDXL use
 * (models/unet_2d_condition.py:160-215). */
typedef struct rt_config {
    int n_levels;
    int block_out_channels[RT_MAX_LEVELS];
    int down_has_attn[RT_MAX_LEVELS];   /* CrossAttnDownBlock2D (1) vs DownBlock2D (0) */
    int up_has_attn[RT_MAX_LEVELS];     /* CrossAttnUpBlock2D (1) vs UpBlock2D (0), in up_blocks order */
    int layers_per_block[RT_MAX_LEVELS];
    int transformer_layers[RT_MAX_LEVELS];
    int heads[RT_MAX_LEVELS];           /* `attention_head_dim` of the config = number of heads */
    int cross_attention_dim;
    int norm_groups;
    float norm_eps;
    int use_linear_projection;
    int addition_text_time;             /* addition_embed_type == "text_time" */
    int addition_time_embed_dim;
    int projection_class_embeddings_input_dim;
    int in_channels, out_channels;      /* 4, 4 */
    int latent_h, latent_w;             /* largest latent the workspace is sized for */
    int max_streams;                    /* UNet forwards batched per launch (<= RT_MAX_STREAMS) */
    int max_prompts;                    /* prompts resident in the cross-attention K/V cache (<= 64) */
    int max_keys;                       /* keys of the longest prompt: 77, 154 or 231 = one, two or three 77-token CLIP windows (0 = 77).  Sizes the
                                         * K / V^T caches (96 rows per window and prompt), the font-size tables and the cross-map store; what a step
                                         * launches depends on the prompts' own key counts only (rt_set_prompts_keys), never on this capacity */
    int ip_tokens;                      /* image tokens per prompt slot (IP-Adapter, rt_set_image_prompts): 0 = no image prompts - what a zero-initialised
                                         * struct gets: nothing new is registered, allocated or launched and the weight table is the reference's
                                         * state_dict layout - or 1 .. 16: every attn2 registers <module>.to_k_ip.weight / .to_v_ip.weight
                                         * [heads d, cross_attention_dim] (packed like to_k / to_v, in the same arena) and keeps two more caches of
                                         * 16 rows per prompt slot */
    int controlnet;                     /* 1: the engine holds one ControlNet (rt_set_control_hint / rt_set_control_scales): a second copy of the
                                         * UNet's encoder registered under the prefix "controlnet." in diffusers' ControlNetModel layout, in the same
                                         * arena behind the UNet's own weights.  0 - what a zero-initialised struct gets - : nothing new is
                                         * registered, allocated or launched and the weight table is the reference's state_dict layout */
    int control_hint_channels;          /* channels of the hint image (0 = 3) */
    int control_embed_channels[4];      /* channels of the hint embedder's four stages (all 0 = 16, 32, 96, 256); each a multiple of 8 */
    int lora_rank;                      /* rank columns R of the regional LoRA adapters (rt_set_lora_scales; csrc/lora.hip): 0 = none - what a
                                         * zero-initialised struct gets: nothing new is registered, allocated or launched and the weight table is the
                                         * reference's state_dict layout - or a multiple of 16 up to 128: each of the eight attention projections
                                         * attn{1,2}.{to_q,to_k,to_v,to_out.0} of every transformer block of the main UNet (never the ControlNet copy)
                                         * registers lora.<module>.down.weight [R, K], lora.<module>.up.weight [N, R] and
                                         * lora.<module>.alpha_over_rank [R] in the same arena, packed like the base weight they sit beside, and the
                                         * engine keeps the padded bf16 prompt embeddings (max_prompts * 96 * max_keys / 77 rows) for the attn2 caches */
    int lora_targets;                   /* the modules regional LoRA adapts (lora_rank > 0): 0 = the eight attention projections, the weight table
                                         * above, bit for bit; 1 = also ff.net.0.proj [8C, C] (its `up` [8C, R] packed in the base weight's GEGLU row
                                         * order, per 64 rows [32 value | 32 gate]), ff.net.2 [C, 4C] of every transformer block and proj_in /
                                         * proj_out [C, C] of every Transformer2DModel of the main UNet (linear or 1x1 convolution: the factors are
                                         * registered 2-D), each with the same three lora.<module>.* slots, packed plainly */
} rt_config;

typedef struct rt_engine rt_engine;

/* lifecycle -------------------------------------------------------------------------------------- */
int rt_create(const rt_config* cfg, int device, rt_engine** out);   /* RegionDiffusion.__init__ rd.py:16-47, xl.py:56-134 */
int rt_destroy(rt_engine* e);
const char* rt_last_error(rt_engine* e);                             /* e may be NULL: last error of failed rt_create */
int rt_set_stream(rt_engine* e, void* hip_stream);   /* NULL: back to the stream rt_create made.  A step call is hipGraph-capturable on it (tests/test_engine_gpu.py) */
int rt_synchronize(rt_engine* e);

/* weights: names are the reference UNet's state_dict keys (unet.load_state_dict, rd.py:32, xl.py:115) --- */
int rt_weight_count(rt_engine* e);
int rt_weight_info(rt_engine* e, int idx, char* name, int name_cap, int64_t* shape4, int* ndim);
/* A weight may be bound again at any time (LoRA, tests): everything the engine derives from it follows - packed forms at once, the
 * LayerNorm-folded projections at the next forward.  Re-binding a weight that rt_set_prompts reads (attn2.to_k / to_v, to_k_ip / to_v_ip,
 * add_embedding.*) - and rt_arena_mark_bound - discards the prompts: call rt_set_prompts again before the next forward or step. */
int rt_bind_weight(rt_engine* e, const char* name, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
int rt_weights_missing(rt_engine* e, char* buf, int cap);            /* returns count; names ';'-joined into buf */
int rt_arena_info(rt_engine* e, void** dev_ptr, uint64_t* bytes);    /* packed arena, for one RCCL broadcast */
int rt_arena_mark_bound(rt_engine* e);                               /* after the arena was filled by a broadcast */

/* per image -------------------------------------------------------------------------------------- */
/* text conditioning: prompt_embeds [P,77,D] f32, pooled [P,Dp] f32 (SDXL) or NULL, time_ids[6] (host) or NULL.
 * rd.py:49-84 / xl.py:256-442,741-762; index 0 = negative prompt, 1..P-2 = region prompts, P-1 = base prompt */
int rt_set_prompts(rt_engine* e, const float* prompt_embeds, const float* pooled, const float* time_ids_host,
                   int n_prompts, int pooled_dim);
/* Prompts of different lengths (no counterpart in the reference, whose processor asserts 77 keys: attention_processor.py:386): prompt_embeds
 * [P, L, D] f32 with L = 77 c; prompt p's first key_counts_host[p] rows are its keys - a multiple of 77, <= L and <= rt_config.max_keys - and
 * the rest of its L rows is ignored (a shorter prompt is NOT padded with empty windows: it attends over exactly its own keys).  A count
 * above max_keys is RT_E_INVALID, nothing is computed and the engine stays usable.  rt_set_prompts == L = 77, every count 77. */
int rt_set_prompts_keys(rt_engine* e, const float* prompt_embeds, const int* key_counts_host, int L, const float* pooled,
                        const float* time_ids_host, int n_prompts, int pooled_dim);
/* Image prompts by decoupled cross-attention (IP-Adapter; no counterpart in the reference).  Engines with rt_config.ip_tokens > 0 only.
 * Slot p is the text prompt slot p of rt_set_prompts: a stream uses the image of the prompt it runs, in every stream mode and in the
 * split steps alike.  tokens [n_prompts, ip_tokens, D] f32 on the device = the PROJECTED image tokens in cross-attention space (may be
 * NULL when every scale is 0); counts_host[p] in 1 .. ip_tokens = the valid tokens of slot p (NULL: all); scales_host[p] finite, 0 = prompt
 * p has no image.  Every attn2 then computes
 *   O = attn(Q, K_text, V_text) + scale[p] attn(Q, to_k_ip(tokens[p]), to_v_ip(tokens[p]))        two separate softmaxes
 * with the image term added into the attention output in place by one more launch (csrc/ipattn.hip) in front of to_out; it runs only for
 * the streams whose prompt has scale != 0 - every other stream, and every launch without one, keeps the bits it has without this call.
 * The token-map store records the text probabilities only.  Slots n_prompts .. are switched off.  rt_set_prompts / rt_set_prompts_keys
 * reset every scale to 0 (the slots change meaning); every other call leaves the state alone.  n_prompts above the prompts set, a count
 * out of range, a non-finite scale or an engine with ip_tokens == 0: RT_E_INVALID, the state is unchanged and the engine stays usable. */
int rt_set_image_prompts(rt_engine* e, const float* tokens, const int* counts_host, const float* scales_host, int n_prompts);
/* ControlNet (no counterpart in the reference; diffusers' ControlNetModel, restated in tests/controlnet_ref.py - parity with diffusers is
 * unpinned).  Engines with rt_config.controlnet == 1 only; on any other engine the three calls are RT_E_INVALID.
 * rt_set_control_hint: hint [hint_channels, 8 h, 8 w] f32 on the device, values as the checkpoint expects (usually 0 .. 1), h x w = the latent
 *   grid of the forwards it will steer (at most the plan's).  Runs controlnet_cond_embedding once - conv_in, blocks.0 .. 5 (3x3, pad 1; the odd
 *   ones stride 2), SiLU behind each, conv_out without - in fp32 (csrc/control.hip, control_conv3_kernel), and caches the result,
 *   [h w, block_out_channels[0]], which a step adds to controlnet.conv_in(x) of every controlled stream.  Once per image, outside the step:
 *   it allocates and synchronises.  hint == NULL clears the hint.  The hint survives every other call.  A forward or step whose latent grid
 *   differs from the hint's while a stream is controlled is RT_E_INVALID before anything is launched - never a resize.
 * rt_control_embedding_read: copies the cached embedding to dst_dev as f32 [h w, C0] (dst_dev may be NULL: sizes only; rows = 0: no hint).
 * rt_set_control_scales: one finite scale per prompt slot of rt_set_prompts (slots n_prompts .. are 0); 0 = a stream that runs that prompt
 *   is not controlled.  rt_set_prompts / rt_set_prompts_keys reset every scale to 0; the hint stays.  A bad argument leaves the state alone.
 * With a hint set, every stream b of a forward whose slot has a scale != 0 is controlled: the control copy runs for those streams only, in
 * stream order, on the stream's own latents, input scale, timestep and prompt (its own key count) - plain softmax, its own Q / K, no
 * injection, no token-map store, no image-prompt term, no FreeU - behind the main UNet's mid block; each of its skips and its mid output
 * goes through its 1x1 zero convolution into fp32 scratch (released before the next), and ONE launch per residual computes
 *   skip[b] <- f16(fmaf(scale[slot(b)], r[b'], float(skip[b])))
 * in place on the main UNet's fp16 skip / mid output (the skip's other reader, the down path, is behind it in stream order).  A stream
 * with scale 0, and a call with no hint or all scales 0, launches nothing new and keeps the bits of an engine without a ControlNet. */
int rt_set_control_hint(rt_engine* e, const float* hint, int h, int w);
int rt_control_embedding_read(rt_engine* e, float* dst_dev, int* rows, int* cols);
int rt_set_control_scales(rt_engine* e, const float* scales_host, int n_prompts);
/* Regional LoRA (rt_config.lora_rank = R > 0; csrc/lora.hip): low-rank adapters kept UNMERGED and scaled per prompt slot.  The factors are
 * ordinary weights (lora.<module>.down.weight / .up.weight / .alpha_over_rank, bound like any other; up to 4 adapters concatenated along
 * the rank, each block zero-padded to a multiple of 16 columns, pad columns with alpha_over_rank 0).
 * rt_set_lora_columns: the adapter (0 .. 3) every rank column belongs to, R host ints (all 0 after rt_create); the same for every module.
 * rt_set_lora_scales: scales_host [n_prompts][4], one finite scale per prompt slot of rt_set_prompts and adapter (slots n_prompts .. are
 *   0).  rt_set_prompts / rt_set_prompts_keys reset every scale to 0.  A bad argument (n_prompts, a non-finite scale, an engine without
 *   adapters or without its weights) returns RT_E_INVALID / RT_E_STATE with the state unchanged.
 * Stream b of a forward whose slot has a non-zero scale computes, on each of the eight projections, y = W x + bf16(f_b (x down^T)) up^T
 * with f_b[j] = scale[slot(b)][adapter(j)] * alpha_over_rank[j] in fp32 (rt_op_lora_add), in place behind the projection's GEMM:
 *   attn1 to_q / to_k (streams some stream attends with: an injected region stream attends with text_ref's Q and K, so its own to_q /
 *   to_k adapters are moot while its to_v and to_out adapters act), to_v (into V^T), attn2 to_q, both to_out.0 (into the fp16 trunk: a
 *   second rounding of the adapted rows, like the ControlNet add).  attn2 to_k / to_v cost nothing in a step: rt_set_lora_scales rebuilds
 *   the K / V^T caches of the main UNet with the GEMMs of rt_set_prompts (same bits) and adds the term to the 96-row blocks of the slots
 *   with a non-zero scale; all scales back to 0 leaves the bits rt_set_prompts left.
 * With rt_config.lora_targets = 1 the term is added in place behind proj_in, ff.net.2 (both into the fp16 trunk) and proj_out as well, and
 *   ff.net.0.proj of an adapted stream runs unfused and once: LayerNorm 3 of its rows, the plain weight into fp32 scratch (one stream's
 *   pre-activations at a time, planned by the dry forward), then rt_op_lora_geglu's kernel into the stream's rows of the GEGLU output; the
 *   other streams of that forward keep the fused GEGLU launch, over the maximal runs of un-adapted streams, and its bits.
 * A stream whose slot has all-zero scales is in no new launch and keeps its bits; an adapted stream's bits do not depend on its
 * neighbours; with every scale 0 no new kernel is launched.  The ControlNet copy runs without adapters.  Nothing is allocated in a step,
 * which stays capturable. */
int rt_set_lora_columns(rt_engine* e, const int* col_adapter_host, int R);
/* Test seam: the device addresses of the attn2 K / V^T caches of transformer block idx of the main UNet (0 .. rt_attn_module_count / 2 - 1, in
 * execution order; [max_prompts * KP, H * DP] and [H * DP, max_prompts * KP] bf16, bytes_each bytes each) - what rt_set_prompts fills and
 * rt_set_lora_scales adapts. */
int rt_attn_cache_info(rt_engine* e, int idx, void** kcache, void** vtcache, long long* bytes_each);
int rt_set_lora_scales(rt_engine* e, const float* scales_host /* [n_prompts][4] */, int n_prompts);
/* Perturbed-attention guidance, scaled per prompt slot (no counterpart in the reference; [memory] diffusers' enable_pag / pag_scale /
 * pag_applied_layers with PAGCFGIdentitySelfAttnProcessor2_0 - parity with it is unpinned; csrc/pag.hip).  A slot with sigma != 0 gets a
 * TWIN of the conditional stream that runs it: one more stream of the step's one batched forward, behind all existing streams, with its
 * partner's latents, input scale, prompt slot, font-size flag, Q / K source, ResNet-feature source, image-prompt term, LoRA scales and
 * ControlNet treatment.  At every APPLIED attn1 module the twin's attention output is O = V = to_v(norm1(x)), head for head - no Q, no
 * K, no softmax; to_out.0 and the residual follow as usual - and at every other module it is an ordinary stream (the twin of an injected
 * region stream still attends with text_ref's Q / K there and takes its ResNet feature).  With T_r the prediction of the stream of slot
 * r, P_r its twin's and m_r its mask:
 *   eps = u + g (sum_r m_r T_r - u) + sum_r m_r sigma_r (T_r - P_r)
 * computed as ONE launch ahead of the step's epilogue, eps[s] <- fmaf(sigma / g, eps[s] - eps[twin], eps[s]) (sigma / g formed in fp32 on
 * the host), after which the unchanged two-term guidance is the three-term formula; v-prediction composes (everything is linear).  The
 * stepped reference pair gets the plain pass's treatment with the base slot's sigma: u_ref + g (T_ref - u_ref) + sigma_base (T_ref - P_ref).
 * rt_set_pag_layers: ';'-joined attn1 module names as rt_attn_module_info lists them (NULL / "": none).  Needs no device; survives every
 *   other call.  An unknown name, an attn2 name, or an empty set while a slot has sigma != 0 is RT_E_INVALID naming the offender.
 * rt_set_pag_scales: one finite sigma per prompt slot of rt_set_prompts (slots n_prompts .. are 0), the calling pattern of
 *   rt_set_control_scales: slot 0 is the negative prompt - it has no twin, a non-zero value is refused -, the rich pass runs region r on
 *   slot r + 1 and the base prompt (base stream, and text_ref while the pair is stepped) on the last slot, the plain pass its text on slot
 *   1.  rt_set_prompts / rt_set_prompts_keys reset every sigma to 0.  A bad argument leaves the state alone.
 * Stream order of a rich step: [uncond, base, uncond_ref, text_ref, regions ..., twin of base, twin of text_ref (only while the pair is
 * stepped), twins of the regions with sigma != 0]; of a plain step: [uncond, text, twin of text].  rt_region_step_part's plan_info[0]
 * counts the twins; the split keeps text_ref, the regions and every twin in the last range while the injection is on, and the plain twin
 * rides with the text stream's part.  More streams than rt_config.max_streams is RT_E_INVALID naming both numbers.  Refused before any
 * launch, the engine staying usable: guidance_scale == 0 and guidance_rescale > 0 with a sigma != 0 (the rescale needs the unfolded text
 * prediction; rt_plain_step_part takes no guidance scale, so in the split plain step it refuses the rescale and guidance_scale == 0 is
 * refused by rt_plain_step_finish, ahead of its own launches), and a forward whose applied module has a token count that is no multiple of 8 (RT_E_UNSUPPORTED).
 * All sigma 0: no twin exists, no new kernel is launched, every stream keeps its bits; a non-twin stream's bits never depend on whether
 * twins are present.  Nothing is allocated in a step, the entry lists travel in the kernel arguments, a step stays capturable. */
int rt_set_pag_layers(rt_engine* e, const char* names);
int rt_set_pag_scales(rt_engine* e, const float* scales_host, int n_prompts);
/* region masks (model.masks, rd.py:97,119-128 / xl.py:775,810-821): [R,4,h,w] f32 */
int rt_set_masks(rt_engine* e, const float* masks, int n_regions, int h, int w);
/* font-size control (text_format_dict['word_pos'|'font_size'], richtext_utils.py:188-209): HOST arrays; n = 0 disables.
 * word_pos < max_keys: key positions of the base prompt (window c at 77 c + [0, 77)); a position beyond a stream's own key count has no
 * effect on that stream */
int rt_set_fontsize(rt_engine* e, const int64_t* word_pos_host, const float* font_size_host, int n);
/* scheduler tables (HOST arrays): Euler: sigmas[n+1], timesteps[n]; PNDM: alphas_cumprod[1000], timesteps[n_iter];
 * DPM-Solver++: alphas_cumprod[1000], timesteps[n] (integers, descending).
 * The stochastic kinds take their parents' tables: RT_SCHED_EULER_A (4) Euler's sigmas[n+1] / timesteps[n]; RT_SCHED_DPMPP_SDE_1 / _2
 * (5 / 6) DPM-Solver++'s alphas_cumprod[1000] / timesteps[n] */
int rt_set_schedule(rt_engine* e, int kind, const float* timesteps_host, int n_timesteps, const float* table_host,
                    int n_table, int num_inference_steps);
/* Seed of the noise field of the stochastic kinds (csrc/philox.h: Philox4x32-10, key = the seed's two words, counter = (pixel, step index,
 * 0, 0), one call per pixel = its four channels).  Engine state, default 0; survives rt_set_schedule and rt_set_latents; the three
 * deterministic kinds ignore it.  The same seed gives the same field on every rank, in the plain pass and in both streams of a rich step. */
int rt_set_noise_seed(rt_engine* e, unsigned long long seed);
/* What the UNet predicts and how the guidance is rescaled (no counterpart call in the reference: `guidance_rescale` is an argument of
 * sample(), xl.py:42-53, :903-905; v-prediction is the checkpoint's scheduler_config.json).  prediction_type RT_PRED_EPSILON (0) or
 * RT_PRED_V (1); guidance_rescale = phi in [0, 1].  Engine state, default (0, 0); survives rt_set_schedule and rt_set_latents; other values
 * are RT_E_INVALID and leave the state alone.  With (0, 0) a step launches exactly what it launched before this call existed.  Otherwise
 * rt_region_step / rt_*_step_finish / rt_plain_step run the two launches of csrc/guided.hip before the unchanged epilogue:
 *   cfg  = the mask-composed, guided prediction (the pair: its own CFG),   text = its conditional half
 *   f    = phi std(text) / std(cfg) + (1 - phi)     std over all 4 h w values, unbiased, fp64 sums in a fixed order, f rounded to fp32 once;
 *                                                   the main stream and the reference pair each use their own two series
 *   m    = cfg f                                    (phi > 0)
 *   eps  = cv m + cx x                              (v; x = the stream's unscaled latents; sigma space: cv = 1 / sqrt(sigma^2 + 1),
 *                                                   cx = sigma / (sigma^2 + 1); VP: cv = sqrt(ac_t), cx = sqrt(1 - ac_t))
 * and the scheduler update, its history and the noise_pred of rt_get_state_ptrs see eps.  Every rank of a split step computes the same bits. */
enum { RT_PRED_EPSILON = 0, RT_PRED_V = 1 };
int rt_set_prediction(rt_engine* e, int prediction_type, float guidance_rescale);
/* FreeU (no counterpart in the reference; diffusers >= 0.21 `pipe.enable_freeu(s1, s2, b1, b2)`, same argument order): in front of EVERY
 * resnet of up block i in {0, 1} - before the concatenation feeds GroupNorm, conv1 and the shortcut - with (b, s) = (b1, s1) / (b2, s2):
 *   hidden[:, :, c] <- fp16(fp32(hidden[:, :, c]) b)            for c < C1 / 2
 *   skip[y, x]      <- skip[y, x] + (s - 1) / (H W) Re( sum_{(ky, kx) in {-1, 0}^2} fftn(skip)[ky, kx] exp(2 pi i (ky y / H + kx x / W)) )
 * per stream and channel (fourier_filter with its fixed threshold = 1: the four lowest bins times s), fp32, one rounding to fp16; every
 * stream of a forward alike, each a function of that stream alone.  All four finite and > 0, else RT_E_INVALID and the state stays.
 * Engine state, default (1, 1, 1, 1) = off: a forward then launches exactly what it launched before this call existed; s == 1 launches no
 * filter and b == 1 no scaling for that block.  Survives every other call.  While enabled, a forward whose deepest grid has a side < 2
 * is RT_E_UNSUPPORTED before anything is launched.  csrc/freeu.hip. */
int rt_set_freeu(rt_engine* e, float s1, float s2, float b1, float b2);
/* sampler state: latents [1,4,h,w] f32 (copied in); the reference stream starts as a clone (rd.py:93, xl.py:774) */
int rt_set_latents(rt_engine* e, const float* latents, int h, int w);
int rt_get_latents(rt_engine* e, float* latents_out, float* latents_ref_out /* may be NULL */);
/* image start (no counterpart in the reference, whose loops start from noise: rd.py:91-93, xl.py:766-774).  x0 [4,h,w] f32 (encoded
 * image, already scaled), noise [4,h,w] f32, keep [h,w] f32 in [0,1] or NULL (nothing pinned): copied into buffers the engine owns,
 * allocated here and never inside a step.  x0 == NULL clears the source. */
int rt_set_source(rt_engine* e, const float* x0, const float* noise, const float* keep, int h, int w);
/* latents = a*x0 + b*noise, the reference stream the same values (as rt_set_latents clones); resets the sampler state like rt_set_latents.
 * (a, b) = the scheduler's start level (schedulers.py start_level()).  RT_E_STATE without a source. */
int rt_noise_latents(rt_engine* e, float a, float b);
/* latents = keep*(a*x0 + b*noise) + (1 - keep)*latents: pins the kept pixels to the source at the level the step just reached
 * (schedulers.py source_levels()).  One elementwise launch on the engine's stream (hipGraph-capturable), touches the latents only, not the
 * reference stream.  RT_E_STATE without a source; a no-op when the source has no keep mask.  fp32 order: csrc/step.hip. */
int rt_source_blend(rt_engine* e, float a, float b);

/* hot path ---------------------------------------------------------------------------------------- */
/* one iteration of the rich-text loop (rd.py:99-173 / xl.py:779-872 without colour guidance):
 * all R+1 / R+3 UNet forwards batched, mask combine, CFG, scheduler step, background blend */
/* inject_selfattn / inject_background are DOUBLES: the reference evaluates `t > (1-inject_selfattn)*1000` and
 * `int(inject_background*len(timesteps))` on Python floats (rd.py:103-104, xl.py:783-784); float32 would move the blend step
 * by one for e.g. 0.7 x 50 steps */
int rt_region_step(rt_engine* e, int step_index, float guidance_scale, double inject_selfattn, double inject_background,
                   int xl_semantics, int flags /* bit 0: elide reference forwards that cannot influence the output;
                                                  bit 1: defer the background blend to rt_background_blend() */);
/* the deferred blend of the last step (colour guidance sits between the scheduler step and the blend: rd.py:151-173) */
int rt_background_blend(rt_engine* e);
/* Intra-image split of one rich-text step over `nparts` GPUs (the F forwards at region_diffusion_sdxl.py:787-821 are
 * independent except that injected region forwards consume the text_ref forward's self-attention Q / K and ResNet feature).  Every
 * rank holds the same engine state and calls, per step:
 *   rt_region_step_part(..., part, nparts, &first, &count)   the UNet forwards of ITS contiguous range [first, first + count) of the
 *                                                            step's stream list [uncond, base, uncond_ref, text_ref, regions...];
 *                                                            text_ref and the region streams always share the last range, so nothing
 *                                                            crosses GPUs inside the forward
 *   (exchange the ranges of the eps buffer, rt_eps_info: stream s at byte offset s * bytes_per_stream - one collective per rank)
 *   rt_region_step_finish(...)                               mask combine + CFG + scheduler step + blend on all streams (every rank)
 * Same arguments / flags as rt_region_step; the result is bit-identical with rt_region_step on one GPU. */
int rt_region_step_part(rt_engine* e, int step_index, float guidance_scale, double inject_selfattn, double inject_background, int xl,
                        int flags, int part, int nparts, int* first_stream, int* n_streams,
                        int* plan_info /* optional [3]: streams of the step, its text_ref stream (-1: none), injection on: the arguments
                                          of rt_op_split_range, from which a rank derives the OTHER ranks' ranges without a collective */);
int rt_region_step_finish(rt_engine* e, int step_index, float guidance_scale, double inject_selfattn, double inject_background, int xl,
                          int flags);
int rt_eps_info(rt_engine* e, void** dev_ptr, unsigned long long* bytes_per_stream, int* max_streams);
/* host-only: the stream range of `part` for a step of n_streams streams whose text_ref stream is text_ref_stream (-1: none) */
int rt_op_split_range(int n_streams, int text_ref_stream, int inject, int part, int nparts, int* first_stream, int* n_streams_out);
/* one iteration of the plain-text loop (rd.py:200-214 / xl.py:880-905): batch-2 forward, CFG, step */
int rt_plain_step(rt_engine* e, int step_index, float guidance_scale);
/* The same step shared by the ranks of a process group (round 6; sample.py --gpus N --split_image): part 0 runs the unconditional forward,
 * part 1 the text forward - and is the rank whose engine records the token maps -, further parts none ([first, first + count) of the
 * stream list [uncond, text]); the ranks exchange their slots of the eps buffer (rt_eps_info) and every rank calls rt_plain_step_finish
 * (CFG + scheduler step).  Bit-identical with rt_plain_step on one GPU. */
int rt_plain_step_part(rt_engine* e, int step_index, int part, int nparts, int* first_stream, int* n_streams);
int rt_plain_step_finish(rt_engine* e, int step_index, float guidance_scale);
/* host-only: the streams of a plain step as the state stands - 2, or 3 with a perturbed twin of the text stream (rt_set_pag_scales), which
 * rides with the text stream's part: ranges (0, 1), (1, n - 1), (n, 0) ... */
int rt_plain_streams(rt_engine* e, int* n_streams);

/* token-map attention store (hooks rd.py:397-443, xl.py:959-1016): head-averaged softmax(QK^T) of the
 * CONDITIONAL stream of rt_plain_step, recorded for the named attention modules (reference module names such as
 * "down_blocks.1.attentions.0.transformer_blocks.0.attn1").  mode 1: accumulate over calls after the module's 10th
 * call (n_maps[name] > 10); mode 2: overwrite after the 10th call (the SD-v1.5 self-attention quirk, rd.py:423);
 * mode 0: off.  A cross-attention map has as many columns as the recorded prompt has keys (77, 154 or 231).  Self-attention maps are limited to 32x32 tokens (the only ones get_token_maps consumes). */
int rt_attn_store_enable(rt_engine* e, const char* module_name, int mode);
int rt_attn_store_reset(rt_engine* e);
int rt_attn_store_read(rt_engine* e, const char* module_name, float* dst_dev /* [rows, cols] f32 or NULL */, int* n_calls,
                       int* rows, int* cols);
int rt_attn_module_count(rt_engine* e);
int rt_attn_module_info(rt_engine* e, int idx, char* name, int name_cap, int* max_tokens, int* heads);

/* per-launch HIP-event timing of the MFMA kernels on the engine's stream (bench.py roofline leg).
 * Algorithmic FLOPs are counted per launch (2*M*N*K for GEMM/conv, 4*B*H*N*NK*d for attention; padded
 * head dims / keys are not counted). */
enum { RT_PROF_GEMM_DENSE = 0, RT_PROF_GEMM_CONV = 1, RT_PROF_ATTN_SELF = 2, RT_PROF_ATTN_CROSS = 3,
       RT_PROF_ATTN_STORE = 4 /* head-averaged map accumulation of the plain pass (attn_store_kernel, HBM-side accumulators); the
                                  * elementwise class, priced in bytes: the FreeU launches of rt_set_freeu are counted here too */,
       RT_PROF_XATTN_FUSED = 5 /* to_q + 77-key cross-attention as one launch (gemm16 EPI_XATTN): FLOPs = 2*M*HD*C + 4*B*H*N*77*d */,
       RT_PROF_XBLOCK = 6 /* the whole cross-attention block as one launch (xblock.hip): FLOPs = 4*M*HD*C + 4*B*H*N*77*d */,
       RT_PROF_IP_ATTN = 7 /* the image-prompt term of attn2 (ipattn.hip; rt_set_image_prompts): FLOPs = 4*H*N*d*(image tokens of the launch's
                            * streams), bytes = Q read once + O read and written once for the streams that carry an image */,
       RT_PROF_CONTROL_ADD = 8 /* the ControlNet residual add (control.hip; rt_set_control_scales), priced in bytes: the fp32 residual read once, the
                                * fp16 skip read and written once, for the controlled streams */,
       RT_PROF_LORA = 9 /* the regional LoRA term of one projection (lora.hip; rt_set_lora_scales), for the adapted streams of the launch:
                         * FLOPs = 2 * rows * R * (K + N), bytes = X read once + Y read and written once (ff.net.0.proj's kernel: X and the
                         * fp32 pre-activations read once, the GEGLU output written once) */,
       RT_PROF_PAG = 10 /* perturbed-attention guidance (pag.hip; rt_set_pag_scales), priced in bytes: the identity attention of the twins at an
                         * applied module (V^T read, O written once) and the fold of a step (partner read and written, twin read) */ };
int rt_profile_enable(rt_engine* e, int on);     /* on: start recording (clears old records); off: stop */
int rt_profile_read(rt_engine* e, int kernel_class, int* count, double* total_ms, double* total_flops);
/* as rt_profile_read, plus the ALGORITHMIC HBM bytes of the launches (attention store: the fp32 accumulator read + written once and the
 * Q / K rows of the recorded stream read once; 0 for the classes that are priced in FLOPs) */
int rt_profile_read2(rt_engine* e, int kernel_class, int* count, double* total_ms, double* total_flops, double* total_bytes);

/* operator level (parity tests, AttnProcessor / unet(...) seams; unet_2d_condition.py:703-717) ------------ */
/* x [B,4,h,w] f32 NCHW; per-stream: input scale, prompt index, font-size flag, self-attention Q/K source
 * stream (== own index for normal attention), resnet-feature source stream or -1; out [B,4,h,w] f32 NCHW */
int rt_unet_forward(rt_engine* e, const float* x, int B, int h, int w, float timestep, const float* in_scale_host,
                    const int* prompt_idx_host, const int* fontsize_host, const int* qk_src_host,
                    const int* res_src_host, float* out);
/* Trace seam (test infrastructure in the product, like the rt_op_* entries): the SAME forward - `out` equals rt_unet_forward's bit for
 * bit - which, when the module `module_name` has finished, copies the trunk tensor that module leaves (fp16 NHWC) to trace_out_dev as
 * fp32 NCHW [B, C, h', w'].  Traceable modules carry the reference's module names: "conv_in", every "...resnets.j", every
 * "...attentions.j" (the whole Transformer2DModel, residual included), every "...downsamplers.0.conv" / "...upsamplers.0.conv" and
 * "conv_out" (whose tensor is `out` itself).  Engines with a ControlNet also list, behind "mid_block.resnets.1" where they run:
 * "controlnet.hint_embedding" (the cached embedding, ONE entry [1, C0, h, w]), "controlnet.<module>" for the control copy's conv_in (hint
 * embedding added), resnets, attentions and downsamplers (the CONTROLLED streams of the call in stream order, [Bc, C, h', w'];
 * RT_E_INVALID when the call controls none), and "controlnet.skip.{k}" / "controlnet.mid": the main UNet's k-th skip / mid output as the
 * up path consumes it, after the add, all B streams.  rt_trace_module_info lists them in execution order with their channel count C and the
 * power of two their grid is smaller than the latent grid by (h' = h >> downshift); it needs no device.  An unknown name or
 * trace_cap_floats < B C h' w' is an error (rt_last_error) before anything is launched or written.  The copy is one plain kernel
 * between the module and its successor; a traced forward is not meant for hipGraph capture. */
int rt_unet_forward_trace(rt_engine* e, const float* x, int B, int h, int w, float timestep, const float* in_scale_host,
                          const int* prompt_idx_host, const int* fontsize_host, const int* qk_src_host, const int* res_src_host,
                          float* out, const char* module_name, float* trace_out_dev, long long trace_cap_floats);
/* rt_unet_forward_trace's arguments plus perturb_host: per stream 1 = the stream is perturbed at the applied modules of rt_set_pag_layers
 * (its attention output there is its V); the perturbed streams trail the list.  module_name == NULL: no trace.  perturb_host == NULL: none. */
int rt_unet_forward_perturbed(rt_engine* e, const float* x, int B, int h, int w, float timestep, const float* in_scale_host,
                              const int* prompt_idx_host, const int* fontsize_host, const int* qk_src_host, const int* res_src_host,
                              float* out, const char* module_name, float* trace_out_dev, long long trace_cap_floats, const int* perturb_host);
int rt_trace_module_count(rt_engine* e);
int rt_trace_module_info(rt_engine* e, int idx, char* name, int name_cap, int* channels, int* downshift);

/* epi: 0 bf16 out | 1 fp32 out (+ fp32 residual) | 2 bf16 out + per-batch-entry time embedding | 3 GEGLU (bf16 out, N/2 columns)
 *      | 4 fp16 out (+ fp16 residual): the UNet's residual trunk (fp32 arithmetic in the epilogue, fp16 in HBM like the reference's
 *        fp16 pipelines).  `res` is fp32 for epi 1 and fp16 for epi 4. */
int rt_op_gemm(const void* A, const void* W, const float* bias, void* out, const void* res, const float* temb,
               int mode, int epi, int M, int N, int K, int lda, int ldw, int ldo, int ldres, int temb_ld,
               int rows_per_batch, int Hin, int Win, int Cin, int Hout, int Wout, void* stream);
/* wset_host (cross only): per batch entry the row of wabs / wsgn [nsets, NK] to multiply the exponentials / probabilities with
 * (attention_processor.py:386-401), or -1 for plain softmax over the keys < nk_valid (no table reads; NULL = set 0 everywhere). */
int rt_op_attention(const void* Q, int ldq, const void* K, int ldk, const void* VT, int ldvt, void* O, int ldo,
                    const int* q_src_host, const int* k_src_host, const int* v_src_host, const int* wset_host,
                    const float* wabs, const float* wsgn, int B, int H, int N, int NK, int nk_valid, int DP, int cross,
                    void* stream);
/* Cross-attention over cached prompts of different lengths, as the engine launches it: K [P*NK, ldk] / VT [H*DP, ldvt] hold NK = 96, 192 or
 * 288 rows per prompt (96 per 77-token window, a prompt's valid keys first); batch entry b attends with prompt_host[b] over its first
 * key_counts_host[b] keys (77, 154 or 231, <= 77 NK / 96) and nothing else - the rows behind them may hold anything finite.  wset_host /
 * wabs / wsgn [nsets, NK] as rt_op_attention (NULL wset = plain softmax everywhere); q_src_host must be NULL (entry b reads its own Q rows).
 * The kernel of an entry follows its OWN key count: where the shape has cross77_kernel (d = 64, N % 64 == 0) the 77-key entries run on
 * it - the bits of rt_op_attention with nk_valid = 77 - and the longer ones on the tile loop of attn_kernel; other shapes: one launch of
 * attn_kernel, every workgroup with the trip count of its entry. */
int rt_op_attention_keys(const void* Q, int ldq, const void* K, int ldk, const void* VT, int ldvt, void* O, int ldo,
                         const int* q_src_host, const int* prompt_host, const int* wset_host, const float* wabs, const float* wsgn,
                         const int* key_counts_host, int B, int H, int N, int NK, int DP, void* stream);
/* The image-prompt term of rt_set_image_prompts alone (csrc/ipattn.hip), in place on the attention output: for batch entry b with slot
 * s = slot_host[b], T = count_host[b] in 1 .. 16 keys and sigma = scale_host[b] (finite), every query n and head h:
 *   p_j = softmax_j(Q[b, n, h, :] . Kip[s, j, h, :]),  j < T        (Q pre-scaled by d^-1/2 log2 e: base-2 exponent; keys T .. 15 masked)
 *   O[b, n, h, :] <- bf16(fp32(O[b, n, h, :]) + sigma sum_j p_j Vip[s, j, h, :])                  one rounding of the sum
 * Q [B N, ldq] and O [B N, ldo] bf16, head h at column h DP; Kip [*, ldk] bf16, row 16 s + j; VTip [H DP, ldvt] bf16, row h DP + d, column
 * 16 s + j.  DP in {32, 64, 96, 128, 160}, N % 8 == 0, leading dimensions % 8 == 0, B <= 16.  slot < 0 or scale == 0: entry b is not
 * launched and keeps its bytes.  Columns whose image term is exactly 0 (the pad columns d .. DP behind zero V^T rows) keep their bits.
 * Each entry is a function of itself alone: deterministic and batch invariant. */
int rt_op_ip_attention(const void* Q, int ldq, const void* Kip, int ldk, const void* VTip, int ldvt, void* O, int ldo,
                       const int* slot_host, const int* count_host, const float* scale_host, int B, int H, int N, int DP, void* stream);
/* The unmerged low-rank (LoRA) term of a projection (csrc/lora.hip), added in place into that projection's output, per stream.  Up to
 * 4 adapters are concatenated along the rank into R rank columns (R % 16 == 0, 16 <= R <= 128; every adapter's block zero-padded to a
 * multiple of 16): down [R, ldd] bf16 (K contiguous), up [N, ldu] bf16 (R contiguous), alpha_over_rank [R] f32 and col_adapter [R] int32
 * (0 .. 3) on the device, 16-byte aligned.  Batch entry b with its rows at row_host[b] (a multiple of 8) and scale_host[4 b + l] for
 * adapter l (finite), f_b[j] = scale_host[4 b + col_adapter[j]] * alpha_over_rank[j]:
 *   T[m, j]  = sum_k X[row_b + m, k] down[j, k]                      bf16 operands, fp32 accumulation
 *   Ts[m, j] = bf16(f_b[j] T[m, j])                                  the fp32 factor is applied BEFORE the one bf16 rounding
 *   Y[m, n]  = round(fp32(Y[m, n]) + sum_j Ts[m, j] up[n, j])        ONE rounding to Y's type
 * form 0: Y bf16 [*, ldy], element (row_b + m, n); form 1: Y bf16 transposed [N, ldy], element (n, row_b + m); form 2: Y fp16 as form 0.
 * X [*, ldx] bf16.  rows % 8 == 0, K % 8 == 0, N % 8 == 0, leading dimensions % 8 == 0, B <= 16.  An entry whose four scales are all 0 is
 * not in the grid and keeps its bytes; with no entry left nothing is launched (*launched, optional: the entries in the grid).  An
 * element whose term is exactly 0 (rows of `up` that are zero: head padding) keeps its bits.  Each row is a function of itself alone:
 * deterministic and batch invariant.  The packed weights carry whatever the base projection's pack carries (head padding, to_q's
 * d^-1/2 log2 e): the kernel knows nothing of heads. */
/* The identity attention of perturbed-attention guidance alone (csrc/pag.hip), in rt_op_attention's layouts: O[b N + n, c] = VT[c, b N + n]
 * for c < H DP and the n batch entries entry_host names (each once, < B); VT [H DP, ldvt] bf16 (row h DP + d, column = token; the pad rows
 * d .. DP are copied like the rest), O [B N, ldo] bf16 (head h at column h DP).  N % 8 == 0, DP as rt_op_ip_attention accepts, leading
 * dimensions multiples of 8, 16-byte aligned pointers.  Entries that are not named keep their bytes.  Bit-exact: a transpose. */
int rt_op_identity_attention(const void* VT, int ldvt, void* O, int ldo, const int* entry_host, int n, int B, int H, int N, int DP, void* stream);
/* The fold of a step alone: eps [n_streams][h w][4] fp32 (rt_eps_info's layout); pair i: eps[stream_host[i]] <- fmaf(ratio_host[i],
 * eps[stream_host[i]] - eps[twin_host[i]], eps[stream_host[i]]).  A stream is named once; a twin's slot is read only. */
int rt_op_pag_fold(float* eps, int n_streams, int h, int w, const int* stream_host, const int* twin_host, const float* ratio_host, int n, void* stream);
int rt_op_lora_add(const void* X, int ldx, const void* down, int ldd, const void* up, int ldu, const float* alpha_over_rank,
                   const int* col_adapter, void* Y, int ldy, int form, const int* row_host, const float* scale_host, int B, int rows, int K,
                   int N, int R, int* launched, void* stream);
/* ff.net.0.proj of adapted streams from the base projection's fp32 pre-activations (csrc/lora.hip, lora_geglu_kernel), in rt_op_lora_add's
 * argument style.  Z [*, ldz] fp32: row (row_b + m) holds the N = 8C pre-activations (bias in) in the packed column order of the GEGLU
 * GEMM, per 64 columns [32 value | 32 gate]; `up` [N, ldu] has its rows in the same order.  With T, Ts as in rt_op_lora_add and D = Ts up^T:
 *   out[row_b + m, 32 blk + c] = bf16( (Z[.., 64 blk + c] + D[.., 64 blk + c]) * gelu(Z[.., 64 blk + 32 + c] + D[.., 64 blk + 32 + c]) )
 * ONE rounding; gelu = the polynomial erf form of the fused GEGLU epilogue.  out [*, ldo] bf16, N / 2 columns.  rows % 8 == 0, K % 8 == 0,
 * N % 64 == 0, R % 16 == 0 in 16 .. 128, ldx / ldd / ldu / ldo % 8 == 0, ldz % 4 == 0, 16-byte aligned pointers, B <= 16; a refusal returns an
 * error and launches nothing.  An entry whose four scales are all 0 is not in the grid and its rows of out are not written; with no
 * entry left nothing is launched.  Each row is a function of itself alone: deterministic and batch invariant. */
int rt_op_lora_geglu(const void* X, int ldx, const void* down, int ldd, const void* up, int ldu, const float* alpha_over_rank,
                     const int* col_adapter, const float* Z, int ldz, void* out, int ldo, const int* row_host, const float* scale_host, int B,
                     int rows, int K, int N, int R, int* launched, void* stream);
/* Host-only (no GPU): the partition of a self-attention launch into shared-probability units (round 6; csrc/attention.hip).  Streams that
 * attend with the same (q_src, k_src) - text_ref and the region streams that take its probabilities, attention_processor.py:522-524 - are dealt
 * G at a time into units that compute softmax(QK^T) once; mode 0 = the shape rule (tokens >= 2048: units of four in their own launch, else
 * pairs beside the one-stream units), 1 = never, 2 - 5 as rt_op_gemm_debug bits 24 - 26.  Per batch entry: launch_of (0 = the G-member
 * kernel's launch, 1 = the separate one-stream launch; 1 for every entry when nothing is shared), unit_of, members_of.  Returns G (0: no sharing),
 * -1 on bad arguments. */
int rt_op_attention_units_plan(const int* q_src, const int* k_src, int B, int tokens, int DP, int mode, int* launch_of, int* unit_of, int* members_of);
/* Host-only query of the shape rule of csrc/gemm16.hip (no device needed; tests/test_gemm16_pick.py): the tile variant a problem of `streams`
 * streams x rows_per_stream rows takes (ids below; -1: not in the family / stays on gemm.hip or the patch convolution; -2: conv3x3 query
 * with a non-square map).  conv3x3 = 1: stride-1 3x3 convolution with Cin = K_or_Cin input channels on a square map of rows_per_stream
 * pixels.  *w_stationary = 1 when the launch uses the W-stationary tile -> XCD order.  The summation CLASS of the answer ({2,3,4,5,8,10,11} /
 * {0,1,9} / {6,7,12} / -1) never depends on `streams`; inside a class the tile shape follows the batch. */
int rt_op_gemm16_pick(int conv3x3, int epi, int streams, int rows_per_stream, int N, int K_or_Cin, int weights_on_rows, int* w_stationary);
/* Host-only query of the split rule of csrc/gemm.hip for problems that cannot fill the chip (no device needed; tests/test_split_plan.py):
 * the route launch_gemm takes (csrc/gemm.hip, gemm_route).
 * *route 0: one launch | 1: K slices of the 128x128 (implicit) GEMM + reduction launch | 2 (round 6): the 16x16-patch convolution kernel
 * split over its input-channel chunks + reduction launch; *slices: how many.  conv3x3: 0 dense (K_or_Cin = K), 1 stride-1 3x3 convolution,
 * 3 the nearest-2x up-sample folded in (rows_per_stream = OUTPUT pixels, a square map).  Route and slice count are functions of ONE
 * stream's shape (a nominal batch of four), never of `streams`: a stream's k order does not depend on the batch. */
int rt_op_split_plan(int conv3x3, int epi, int streams, int rows_per_stream, int N, int K_or_Cin, int* route, int* slices);
/* Host-only query (no device needed; tests/test_gemm_route.py): the route rt_op_gemm takes for exactly these arguments - gemm_route of
 * the GemmArgs rt_op_gemm itself builds (one helper makes them for both: no stream shares, unlike rt_op_split_plan / rt_op_gemm16_pick,
 * which describe the engine's launches) - under the same switches (rt_op_gemm_force_config, rt_op_gemm_debug / _debug2).  A route is a
 * function of the shape, never of a leading dimension or a pointer.
 * *kind: RT_ROUTE_* below; *variant_or_cfg: the tile variant of csrc/gemm16.hip (G16, G16_UP2; ids at rt_op_gemm16_variant), the tile
 * configuration 0..8 of csrc/gemm.hip (TILE), -1 elsewhere; *slices: K slices (KSPLIT) / input-channel chunks (PATCH_SPLIT), 1 elsewhere.
 * Any of the three may be NULL.  RT_E_INVALID for an unknown mode / epilogue or an empty shape. */
enum { RT_ROUTE_TILE = 0        /* one launch of a csrc/gemm.hip tile configuration (dense or implicit-GEMM convolution) */,
       RT_ROUTE_G16 = 1         /* csrc/gemm16.hip: dense, or the stride-1 3x3 convolution on its main loop */,
       RT_ROUTE_G16_UP2 = 2     /* csrc/gemm16.hip: the 2x-upsample convolution as four 2x2 phase convolutions (needs the phase pack:
                                 * rt_op_upconv only, which reports it as *phase_route) */,
       RT_ROUTE_PATCH = 3       /* the 16x16-patch convolution kernel */,
       RT_ROUTE_PATCH_SPLIT = 4 /* ... split over its input-channel chunks + reduction launch */,
       RT_ROUTE_KSPLIT = 5      /* K slices of the 128x128 (implicit) GEMM + reduction launch */,
       RT_ROUTE_TRIPLE = 6      /* the precise VAE's hi / lo contraction as three launches (rt_vae_* and rt_op_gemm_hilo) */ };
int rt_op_gemm_route(int mode, int epi, int M, int N, int K, int lda, int ldw, int ldo, int rows_per_batch, int Hin, int Win, int Cin,
                     int Hout, int Wout, int* kind, int* variant_or_cfg, int* slices);
/* One tile variant of the 16x16x32-MFMA GEMM family (csrc/gemm16.hip; tests / micro-benchmarks - rt_op_gemm picks by shape):
 * 0: 224x160 K-split  1: 128x160 K-split  2: 224x256  3: 256x256  4: 224x320  5: 256x320  6: 160x224 K-split (V^T)  7: 160x128 K-split
 * 8: 128x256  9: 64x160 K-split  10: 128x320  11: 64x320  12: 160x64 K-split (V^T) - 9..12: the small batches of the plain pass / SD-v1.5;
 * -1: the variant the shape rule picks.  Variants {2,3,4,5,8,10,11} (class A) give the same bits as each other and as every
 * tile configuration of csrc/gemm.hip; {0,1,9} and {6,7,12} (class B: two K halves summed at the end) are bit-identical sets.
 * Dense only, K % 128 == 0, K >= 256; epi as rt_op_gemm (0, 1, 3, 4). */
int rt_op_gemm16_variant(const void* A, const void* W, const float* bias, void* out, const void* res, int epi, int M, int N, int K, int lda,
                         int ldw, int ldo, int ldres, int weights_on_rows, int variant, int wstat, void* stream);
/* attn1's two projections of one LayerNorm output X [M, K] bf16 (models/attention_processor.py:495-506: to_q / to_k / to_v read the same
 * hidden states) exactly as the engine launches them: qk[Mqk, Nqk] = X[:Mqk] Wqk^T + bqk (stacked, head-padded to_q | to_k; Mqk <= M: the
 * injected region streams of a rich-text step need no Q / K of their own) and vt[Nv, M] = Wv X^T.  Where the 16x16x32 family has the pair
 * of tiles (SDXL: both attention levels with 7, 4 and - the plain pass - 2 streams) they go out as ONE grouped launch (csrc/gemm16.hip, gemm16_dual_kernel: the
 * unchanged tile bodies, bit-identical with two launches; rt_op_gemm_debug bit 13 forces two launches); *grouped (may be NULL) says which. */
int rt_op_gemm_pair_pick(int streams_qk, int streams, int rows_per_stream, int Nqk, int Nv, int K);   /* host-only: 0..3 = grouped (which tile pair), -1 = two launches */
int rt_op_gemm_qk_vt(const void* X, int ldx, int K, int rows_per_stream, const void* Wqk, const float* bqk, int Mqk, int Nqk, void* qk, int ldqk,
                     const void* Wv, int Nv, int M, void* vt, int ldvt, int* grouped, void* stream);
/* The SDXL cross-attention block the north star names, as one call (replaces attn2 of BasicTransformerBlock, models/attention.py:169-189,
 * processor arithmetic models/attention_processor.py:476-545, font-size softmax :386-401):
 *   trunk_out[B*N, C] (fp16) = trunk_in + to_out(softmax_fs(to_q(x) K[prompt]^T) V[prompt]) + bo
 * x bf16 [B*N, C] (LayerNorm output); wq bf16 [H*DP, C] head-padded and pre-scaled by d^-1/2 log2 e; wo bf16 [C, H*DP]; bo fp32 [C] or NULL;
 * kcache bf16 [P*96, H*DP], vtcache bf16 [H*DP, ldvt] (77 keys padded to 96 per prompt); prompt_host / wset_host: per batch entry the
 * prompt index and the multiplier set in wabs / wsgn [nsets, 96] (the engine's tables: 0 plain softmax, 1 font-size), or -1 = plain softmax
 * over the 77 valid keys without reading the tables (what the engine passes for every stream without a font-size entry: identical bits,
 * fewer instructions); q_scratch, o_scratch bf16 [B*N, H*DP].
 * Launches: where the tiling allows it (DP = 64, H*64 % 320 == 0, N % 128 == 0, C % 64 == 0: the 1280-channel level of SDXL, 60 of its 70
 * blocks) to_q and the attention are ONE kernel (csrc/gemm16.hip, EPI_XATTN: a 128 x 320 tile = 128 queries x 5 heads stays in LDS,
 * q_scratch is not written) followed by the to_out GEMM; otherwise to_q GEMM -> attention -> to_out GEMM. */
int rt_op_cross_attn_block(const void* x, const void* wq, const void* wo, const float* bo, const void* kcache, const void* vtcache, int ldvt,
                           const int* prompt_host, const int* wset_host, const float* wabs, const float* wsgn, const void* trunk_in_f16,
                           void* trunk_out_f16, void* q_scratch, void* o_scratch, int B, int N, int C, int H, int DP, void* stream);
/* in_type: 0 fp32, 1 bf16 (x2 must be NULL), 2 fp16 - the element type of x1 / x2 (the UNet trunk is fp16) */
int rt_op_groupnorm(const void* x1, const void* x2, int in_type, int C1, int C2, int G, int B, int HW,
                    const float* gamma, const float* beta, float eps, int silu, void* out_bf16, void* raw_out_bf16,
                    void* stream);
/* Host-only (no device needed): the form rt_op_groupnorm takes for these arguments, from the launcher's own predicate - 1: one launch
 * (statistics and apply in one kernel), 2: two launches (statistics, then apply); rt_op_gemm_debug bit 23 forces 2.  RT_E_INVALID (< 0) for
 * arguments rt_op_groupnorm would refuse. */
int rt_op_groupnorm_form(int in_type, int C1, int C2, int G, int B, int HW);

/* ---- The VAE's kernels one call at a time (tests/test_vae_ops_gpu.py).  rt_vae_* reaches them only through a whole decode / guidance /
 * encode; these entries issue the same launches from the same argument builders (csrc/vae.h), so they take the routes, chunkings and
 * block counts the VAE takes and no others.  Scratch is allocated and freed per call where an entry needs some (not for hot paths).
 *
 * rt_op_gemm_hilo: the VAE's contraction, out_f32 [M, ldo] = A W^T + A_lo W^T + A W_lo^T (+ bias) (+ res, fp32 [M, ldres]) accumulated in
 * fp32 from bf16 planes (a value v is the pair hi = bf16(v), lo = bf16(v - hi)).  A_lo == W_lo == NULL: the single-pass call A W^T as the
 * default mode issues it (fp32 output).  mode 0 dense (A [M, lda], W [N, ldw]); 1 / 3 / 4: the 3x3 convolution of ONE NHWC image
 * [Hin, Win, Cin] (Cin % 8 == 0, K = 9 Cin, W [N, ldw] tap-major) - stride 1 / behind a nearest-2x up-sample / stride 2 with bottom-right
 * zero padding; M = rows_per_batch = Hout Wout of that mode (RT_E_INVALID otherwise).  out == res is allowed (the backward pass
 * accumulates in place).  pair_lo != NULL (convolutions): the result leaves as its bf16 pair - out_f32 is then the bf16 hi plane [M, ldo],
 * pair_lo the lo plane with the same ldo - where the route can (pair_ok below), else RT_E_UNSUPPORTED and nothing is launched.
 * rt_op_gemm_hilo_route: host-only, the route of that call for hilo = (A_lo != NULL), pair = (pair_lo != NULL) under the current switches.
 * *kind: RT_ROUTE_TRIPLE when the three passes run as three launches, else the route of the ONE launch that runs them; *pass_kind: the
 * route of each of the three launches (TRIPLE), else = *kind; *variant_or_cfg / *slices belong to *pass_kind; *pair_ok: 1 when this
 * problem's route writes pairs (gemm_pair_output_ok).  Any output may be NULL. */
int rt_op_gemm_hilo(const void* A, const void* A_lo, const void* W, const void* W_lo, const float* bias, float* out_f32, void* pair_lo,
                    const float* res, int mode, int M, int N, int K, int lda, int ldw, int ldo, int ldres, int rows_per_batch, int Hin,
                    int Win, int Cin, int Hout, int Wout, void* stream);
int rt_op_gemm_hilo_route(int hilo, int pair, int mode, int M, int N, int K, int lda, int ldw, int ldo, int rows_per_batch, int Hin, int Win,
                          int Cin, int Hout, int Wout, int* kind, int* variant_or_cfg, int* slices, int* pass_kind, int* pair_ok);
/* hi = bf16(x), lo = bf16(x - hi); n % 4 == 0 */
int rt_op_split_bf16(const float* x, void* hi_bf16, void* lo_bf16, long long n, void* stream);
/* GroupNorm (+ SiLU) of x [B, HW, C] (x_bf16: 0 fp32, 1 bf16) as the VAE launches it: chunks by the VAE's rule
 * (rt_op_vae_groupnorm_nchunk(HW) of them), optional low planes out_lo / raw_lo, optional un-normalised copy raw.  stats: caller's
 * [B, nchunk, G, 2] floats; on return stats[b][0][g] = (mean, rstd), which is what the backward reads.
 * Backward wrt x: dx = rstd (dxh - mean_g(dxh) - xh mean_g(dxh xh)) (+ add), dxh = (dA + dA_lo) silu'(y) gamma; stats as the forward left
 * them; any of out (fp32), out_bf16 (+ out_bf16_lo) may be NULL. */
int rt_op_vae_groupnorm_nchunk(int HW);
int rt_op_vae_groupnorm(const void* x, int x_bf16, int C, int G, int B, int HW, const float* gamma, const float* beta, float eps, int silu,
                        void* out_bf16, void* out_lo, void* raw_bf16, void* raw_lo, float* stats, void* stream);
int rt_op_vae_groupnorm_bwd(const void* x, int x_bf16, const void* dA_bf16, const void* dA_lo, const float* stats, const float* gamma,
                            const float* beta, float eps, int silu, int C, int G, int B, int HW, const float* add, float* out,
                            void* out_bf16, void* out_bf16_lo, void* stream);
/* p (+ p_lo) = softmax(scale s) per row of s [rows, cols] fp32; ds (+ ds_lo) = scale P o (dp - rowsum(dp o P)), P = p + p_lo */
int rt_op_softmax_rows(const float* s, void* p_bf16, void* p_lo, int rows, int cols, float scale, void* stream);
int rt_op_softmax_bwd(const void* p_bf16, const void* p_lo, const float* dp, void* ds_bf16, void* ds_lo, int rows, int cols, float scale,
                      void* stream);
int rt_op_transpose_bf16(const void* in, void* out, int R, int C, void* stream);                  /* [R, C] -> [C, R] */
int rt_op_sumpool2x2(const float* in, float* out, int B, int H, int W, int C, void* stream);      /* [B, 2H, 2W, C] -> [B, H, W, C]; C % 4 == 0 */
/* post_quant_conv: out [HW, 8] bf16 (+ out_lo) = W (c_lat lat + c_eps eps) + b per pixel, channels 4..7 zero; lat / eps [4, HW] (eps may be
 * NULL).  Its adjoint + the guidance update: g[c] = gscale sum_o W[o][c] dz[pix][o]; grad_out[c][pix] = g (optional);
 * lat[c][pix] -= g weight mask_all[c][pix] */
int rt_op_pq_conv_fwd(const float* lat, const float* eps, float c_lat, float c_eps, const float* W, const float* b, void* out_bf16,
                      void* out_lo, int HW, void* stream);
int rt_op_pq_conv_bwd_update(const float* dz, int ldz, const float* W, float gscale, float weight, const float* mask_all, float* lat,
                             float* grad_out, int HW, void* stream);
/* Colour loss of the guidance step and its gradient wrt the decoder output img [HWi, ldi] fp32 (3 channels used): dimg [HWi, 8] bf16
 * (+ dimg_lo), channels 3..7 zero; masks [n, HWi], target_dev [n, 3] on the device, 1 <= n <= 16; *loss_dev (device, optional) */
int rt_op_color_loss_grad(const float* img, int ldi, const float* masks, const float* target_dev, int n, int HWi, void* dimg_bf16,
                          void* dimg_lo, float* loss_dev, void* stream);
int rt_op_layernorm(const float* x, const float* gamma, const float* beta, void* out_bf16, int rows, int C, float eps,
                    void* stream);
int rt_op_layernorm_f16(const void* x_f16, const float* gamma, const float* beta, void* out_bf16, int rows, int C, float eps, void* stream);
/* LayerNorm folded into the projection that consumes it (round 6; csrc/gemm16.hip "LNF").  BasicTransformerBlock applies norm1 / norm2 /
 * norm3 in front of attn1 / attn2 / ff (/root/reference/models/attention.py:150,168,181); the engine computes
 *     LN(x) W^T + b = rstd (xb W'^T - mu s) + c,   W' = bf16(gamma W),  s = row sums of W',  c = b + W beta
 * on xb = the UN-normalised trunk as bf16, which the trunk's producer leaves next to the fp16 trunk together with ONE (sum, sum of squares)
 * of xb per token and column tile of its grid (`tile_cols` = 160 or 320 columns), from which (mu, rstd) of a token follow; eps = 1e-5.
 * `partials`: pair-major [C / tile_cols / 2][tokens] float4 = (sum, sumsq) of two neighbouring tiles.
 * rt_op_ln_gemm: W bf16 packed [N, C] (GEGLU: rows interleaved per 64-block [32 value | 32 gate], as rt_op_gemm epi 3);
 *   epi 0: out bf16 [tokens, N] (weights_on_rows = 1: out = [N, tokens], the V^T form) | epi 3: GEGLU, out bf16 [tokens, N / 2];
 *   (xb_bf16, partials) as a producer left them, or both NULL: made here from the fp16 trunk x_f16 [tokens, C] by the stand-alone kernel.
 *   C = 640 or 1280.  RT_E_UNSUPPORTED (-5) when the shape has no folded form (the engine then keeps the LayerNorm launch).
 *   rows_per_stream as rt_op_gemm16_pick.
 * rt_op_gemm_emit_partials: the fp16-trunk GEMM (rt_op_gemm epi 4, optional fp16 residual) that ALSO leaves xb [M, N] bf16 and the
 *   partials of its output rows (N = 640 or 1280; *tile_cols = the width its tile class uses); RT_E_UNSUPPORTED when the shape's tile
 *   variant has no such epilogue. */
int rt_op_ln_gemm(const void* x_f16, const float* gamma, const float* beta, const void* W_bf16, const float* bias, void* out, int tokens,
                  int N, int C, int epi, int weights_on_rows, int rows_per_stream, const void* xb_bf16, const float* partials, int tile_cols,
                  void* stream);
int rt_op_gemm_emit_partials(const void* A, const void* W, const float* bias, void* out_f16, const void* res_f16, int M, int N, int K,
                             int rows_per_stream, void* xb_bf16, float* partials, int* tile_cols, void* stream);
int rt_op_ln_partials(const void* x_f16, void* xb_bf16, float* partials, int rows, int C, int tile_cols, void* stream);      /* the stand-alone producer of (xb, partials) */
int rt_op_small_linear(const float* a, int lda, const void* W_bf16, int ldw, const float* bias, float* out, int ldo,
                       int B, int N, int K, int silu_in, int accumulate, void* stream);
int rt_op_timestep_embed(const float* t, int n, int dim, float* out, int ldo, void* stream);
int rt_op_cast_bf16(const float* x, void* out_bf16, long long n, void* stream);
/* The FreeU operator of rt_set_freeu alone, in place on fp16 token-major tensors: hidden_f16 [B, H W, C1] (channels < C1 / 2 times b),
 * skip_f16 [B, H W, C2] (the four lowest bins times s).  A NULL pointer skips that half, and so do b == 1 / s == 1 (nothing launched, bytes
 * untouched).  C1, C2 multiples of 8, pointers 16-byte aligned, b, s finite and > 0 (RT_E_INVALID); the filter needs 2 <= H, W <= 2048
 * (RT_E_UNSUPPORTED). */
int rt_op_freeu(void* hidden_f16, int C1, void* skip_f16, int C2, int B, int H, int W, float b, float s, void* stream);
/* The ControlNet residual add alone (csrc/control.hip), in place on skip_f16: for entry i < n, with b = stream_host[i] (distinct, in [0, B)),
 *   skip[b, t, c] <- f16(fmaf(scale_host[i], r[i, t, c], float(skip[b, t, c])))        t < HW, c < C: one fp32 rounding, then one to fp16
 * skip fp16, stream b at skip + b skip_stride elements, token t at + t lds; r fp32, entry i at r + i r_stride, token t at + t ldr.  C % 8 == 0,
 * lds >= C and % 8 == 0, ldr >= C and % 4 == 0, strides and pointers 16-byte multiples, scales finite (RT_E_INVALID otherwise, nothing
 * launched).  Streams that are not named, and every byte outside the [HW, C] windows, are never addressed.  No atomics; an entry is a
 * function of itself alone. */
int rt_op_control_add(void* skip_f16, long long skip_stride, int lds, const float* r, long long r_stride, int ldr, const int* stream_host,
                      const float* scale_host, int n, int B, int HW, int C, void* stream);
/* The noise field a stochastic step with (seed, step index) adds on an h x w latent grid, from the same device function as the step
 * epilogue: out_dev [4, h, w] f32 normals; words_dev [h*w, 4] the raw Philox words of every pixel, or NULL. */
int rt_op_step_noise(unsigned long long seed, int step, int h, int w, float* out_dev /* [4,h,w] */, unsigned int* words_dev /* [h*w,4] or NULL */,
                     void* stream);
/* The pre-pass of rt_set_prediction alone, on caller buffers: eps [F, h*w, 4] f32 (the layout of rt_eps_info), masks [R, 4, h*w] (rich mode),
 * lat / lat_ref [4, h*w] (read only for v-prediction; lat_ref may be NULL without a pair), the stream indices as the step plans them
 * (s_uref < 0: no pair; s_region_host [R - 1], host), `plain`: 1 = eps[s_uncond] + g (eps[s_base] - eps[s_uncond]) without masks, `step_ref`:
 * the pair is stepped.  Outputs: gpred_dev [2][h*w][4] (slot 1 only written when the pair is stepped), factors_dev [2] f32 (1 for the main
 * stream when phi == 0; 0 for the pair when it is not stepped); partials_dev: scratch of ceil(h*w / 256) * 8 doubles (may be NULL when
 * phi == 0). */
int rt_op_guided_prediction(const float* eps, const float* masks, const float* lat, const float* lat_ref, int h, int w, int R, int s_uncond,
                            int s_base, int s_uref, int s_tref, const int* s_region_host, float g, int plain, int step_ref, float phi,
                            int prediction_type, float cv, float cx, float* gpred_dev, double* partials_dev, float* factors_dev, void* stream);
/* ---- CLIP text encoder pieces (transformers' CLIPTextModel[WithProjection] as called at rd.py:53-66, xl.py:330-356); the linear layers
 * and LayerNorms are rt_op_gemm / rt_op_layernorm.  ids [rows] int32 (device), tok [vocab, C], pos [N, C] fp32 -> out [rows, C] fp32 */
int rt_op_embed(const int* ids, const float* tok, const float* pos, float* out, int rows, int N, int C, int vocab, void* stream);
/* kind 0: quick_gelu (CLIP ViT-L), 1: gelu/erf (OpenCLIP bigG); bf16 -> bf16, n elements */
int rt_op_activation(const void* x_bf16, void* out_bf16, long long n, int kind, void* stream);
/* causal self-attention over N <= 128 tokens: q, k, v bf16 [B*N, ld] with head h at column h*d; out bf16 [B*N, ldo] */
int rt_op_causal_attention(const void* q, const void* k, const void* v, int ld, void* out, int ldo, int B, int H, int N, int d, float scale,
                           void* stream);
/* ---- CLIP vision encoder pieces (transformers' CLIPVisionModelWithProjection, the image encoder of IP-Adapter); the patch convolution,
 * the linear layers and the LayerNorms are rt_op_gemm / rt_op_layernorm (rt_op_layernorm: C <= 2048).
 * img_u8 [B, S, S, 3] uint8 RGB (device), S % p == 0 -> out_bf16 [B (S/p)^2, Kp]: column (c p + ky) p + kx = (u / 255 - mean[c]) / std[c] (the
 * flatten order of the conv weight [C, 3, p, p]), columns 3 p^2 .. Kp written as zeros; Kp % 8 == 0, Kp >= 3 p^2; mean / std: 3 host floats */
int rt_op_patchify(const void* img_u8, void* out_bf16, int B, int S, int p, int Kp, const float* mean_host, const float* std_host, void* stream);
/* out [B N, C] fp32 = LayerNorm_{gamma, beta, eps}(e), e[b N] = cls + pos[0], e[b N + 1 + i] = patch[b (N - 1) + i] + pos[1 + i]: patch [B (N - 1),
 * ldp] fp32, cls [C], pos [N, C], gamma / beta [C] fp32; two-pass statistics in fp32; N >= 2, C <= 2048 */
int rt_op_vit_embed(const float* patch, int ldp, const float* cls, const float* pos, const float* gamma, const float* beta, float* out,
                    int B, int N, int C, float eps, void* stream);
/* unmasked self-attention over 1 <= N <= 640 tokens: q, k, v bf16 [B*N, ld] with head h at column h*d; out bf16 [B*N, ldo]; d % 8 == 0,
 * d <= 128, ld % 8 == 0, ldo % 4 == 0, q / k / v 16-byte and out 8-byte aligned.  fp32 scores and online softmax, P rounded to bf16 for
 * the PV product, fp32 accumulation.  Anything else is RT_E_INVALID. */
int rt_op_bidir_attention(const void* q, const void* k, const void* v, int ld, void* out, int ldo, int B, int H, int N, int d, float scale,
                          void* stream);
/* ---- The Resampler of the IP-Adapter "plus" checkpoints (rich_text_to_image_amd/resampler.py); its linear layers, LayerNorms and GELU are
 * rt_op_gemm / rt_op_layernorm / rt_op_activation, rt_op_cast_bf16 in front.  Latent attention: 1 <= Nq <= 16 queries q bf16 [B*Nq, ldq]
 * over 1 <= Nk <= 656 keys / values k, v bf16 [B*Nk, ldkv], head h at column h*d; out bf16 [B*Nq, ldo].  d % 8 == 0, d <= 128, ldq % 8 == 0,
 * ldkv % 8 == 0, ldo % 4 == 0, q / k / v 16-byte and out 8-byte aligned; anything else is RT_E_INVALID before a launch.  One workgroup per
 * (image, head), the keys split over its four waves in tiles of 64, the partial (max, sum, O) merged in wave order without atomics:
 * the same bits on every launch.  Arithmetic as rt_op_bidir_attention: fp32 scores and online softmax in the exp2 domain, P rounded to
 * bf16 for the PV product, fp32 accumulation, one bf16 rounding of the result. */
int rt_op_latent_attention(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, int ldo, int B, int H, int Nq, int Nk, int d,
                           float scale, void* stream);
/* Head-averaged attention probabilities of ONE batch entry (the `attention_probs_avg` the reference processor returns,
 * attention_processor.py:541-545, reshape_batch_dim_to_heads_and_average): out[N, NK] (=|+=) mean_h softmax(Q_h K_h^T).
 * Q rows q_row0+[0,N), K rows k_row0+[0,NKrows) in the rt_op_attention layouts; NK valid keys (any count: processed in chunks of
 * 1024), NKpad = key count padded to a multiple of 32. */
int rt_op_attention_probs_avg(const void* Q, int ldq, long long q_row0, const void* K, int ldk, long long k_row0, float* out,
                              int H, int N, int NK, int NKpad, int NKrows, int DP, int accumulate, void* stream);
/* A recorded layer of the plain pass as the UNet forward runs it: the attention launch over B batch entries (O is written), then the store of
 * batch entry `store_stream` into map_out (=|+= as rt_op_attention_probs_avg).  Where the forward hands the softmax statistics of that entry
 * from the attention launch to the store (stats_ready: the store then runs its apply kernel only) this call does too, by the same
 * predicates; *handover = 1 then, 0 when the store computed its own (rt_op_gemm_debug bit 17 forces that).
 * cross = 0: Q / K [B*N, ld] and V^T as rt_op_attention, entry b attends with Q and K of entry qk_src_host[b] (NULL: its own) and its own V;
 *   NK must equal N; map_out [N, N]; handed over when 256 <= N <= 1024, N % 32 == 0, DP in {32, 64, 96} and qk_src_host[store_stream] == store_stream.
 * cross = 1: K / V^T are prompt caches of NK = 96, 192 or 288 rows per prompt as rt_op_attention_keys (prompt_host, key_counts_host, plain
 *   softmax; wabs / wsgn [1, NK] are read by the generic kernel's argument check only and may be NULL where cross77_kernel runs);
 *   map_out [N, key_counts_host[store_stream]]; handed over when the launch runs on cross77_kernel (d = 64, N % 64 == 0, every entry 77 keys).
 * d = the unpadded head dim. */
int rt_op_attention_store_handover(const void* Q, int ldq, const void* K, int ldk, const void* VT, int ldvt, void* O, int ldo,
                                   const int* qk_src_host, const int* prompt_host, const int* key_counts_host, const float* wabs,
                                   const float* wsgn, int B, int H, int N, int NK, int d, int DP, int cross, int store_stream,
                                   float* map_out, int accumulate, int* handover, void* stream);
/* Host-only query (no device needed; tests/test_cross_route.py): the route of an attn2 launch as the UNet forward decides it - cross_route
 * of csrc/engine.hip, the one function the forward and every entry that launches cross-attention ask - under the current switches
 * (rt_op_gemm_debug bits 4, 16, 17, 19).  The layer: C channels, `heads` heads of dim d padded to DP, `tokens` queries per stream; the
 * prompts: prompt_rows (96, 192 or 288) cached rows each, stream b with key_counts_host[b] = 77, 154 or 231 valid keys; folded: the
 * LayerNorm is folded into to_q; recorded: the layer's token map is enabled in this forward.
 * *kind: RT_CROSS_* below; *handover: 1 when the launch may leave the recorded stream's softmax statistics for the store (what
 * rt_op_attention_store_handover reports for the same arguments; the forward does so from the layer's eleventh recorded call on);
 * stream_kernel (may be NULL) [B]: the kernel that computes stream b - 0 attn_kernel, 1 cross77_kernel, 2 crossmw_kernel, -1 one of the
 * two one-launch forms.  An entry that has no d passes DP (every kernel but attn_kernel needs d = DP = 64).
 * RT_E_INVALID for what rt_op_attention_keys refuses: B outside [1, 16], another prompt_rows, a key count that is not 77 c or exceeds
 * the 77 / 96 of prompt_rows. */
enum { RT_CROSS_GENERIC = 0     /* attn_kernel */,
       RT_CROSS_CROSS77 = 1     /* d = 64, tokens % 64 == 0, every stream 77 keys: cross77_kernel */,
       RT_CROSS_RUNS = 2        /* that shape with different key counts: maximal runs of 77-key streams on cross77_kernel, of longer ones on crossmw_kernel */,
       RT_CROSS_XATTN_FUSED = 3 /* to_q + attention as one launch (PROBES=1 builds) */,
       RT_CROSS_XBLOCK = 4      /* to_q, attention and to_out + residual as one launch (PROBES=1 builds, rt_op_gemm_debug bit 16) */ };
int rt_op_cross_route(int C, int heads, int d, int DP, int tokens, int prompt_rows, const int* key_counts_host, int B, int folded,
                      int recorded, int* kind, int* handover, int* stream_kernel);
const char* rt_op_last_error(void);
/* GEMM tile choice: -1 (default) = a pure function of the problem shape (csrc/gemm16.hip: 16x16x32-MFMA family, 224-row tiles;
 * csrc/gemm.hip: 32x32x16 family for everything else) - no timing, no per-process state; 0..8 = force one tile configuration of
 * gemm.hip (tests / micro-benchmarks; all of them give bit-identical results). */
int rt_op_probes_built(void);      /* 1: the library was built with `make PROBES=1` and contains the measured-and-rejected kernels (xblock_kernel,
                                    * EPI_XATTN, gemm16 variant 13) that rt_op_gemm_debug bits 16 / 4 and variant 13 select; 0: the shipped build */
int rt_op_gemm_force_config(int cfg);
/* A/B switches (benchmarks; the engine wrapper reads RTDIFF_DEBUG_FLAGS once at load); csrc/common.h (DebugBit) names them.  0 = default.
 *  bit 0  patch-eligible 3x3 convs through the implicit-GEMM kernels     bit 1  keep gemm16.hip out
 *  bit 2  no split-K (no K slices, no input-channel chunks)               bit 3  stride-1 3x3 convs stay on the patch kernel (not on gemm16)
 *  bit 4  cross-attention as to_q GEMM + attention launch instead of the fused kernel (probe builds)
 *  bit 5  token-map accumulation on the round-1 two-pass kernel (csrc/attn_store.hip)
 *  bit 6  large token maps on the one-pass kernel instead of the statistics + key-split apply pair
 *  bit 7  the precise VAE's hi / lo contractions as three launches instead of one; bit 8 only those on the gemm16 convolution route,
 *         bit 9 only those on the patch kernel, bit 15 only the DENSE ones
 *  bit 10 chunk-split patch convolutions keep 160-channel column tiles where N % 160 == 0
 *  bit 11 GroupNorm chunks of 128 rows instead of 64                     bit 12 no 5-slot ring for gemm16's 64 x 160 tiles
 *  bit 13 attn1's Q|K and V^T projections as two launches instead of one grouped launch
 *  bit 14 no raised wave priority (s_setprio) in the MFMA phases of the attention kernel
 *  bit 16 the 640-channel cross-attention block as one launch (xblock.hip, opt-in, probe builds)
 *  bit 17 the token-map store computes its softmax statistics itself     bit 18 round 4's token-map apply kernel for every head dim
 *  bit 19 cross-attention on the round-4 kernels instead of cross77_kernel
 *  bit 20 cross77_kernel: one 16-query tile per wave for every shape    bit 21 cross77_kernel: two heads per workgroup
 *  bit 22 LayerNorm launches + bf16 projections instead of the LayerNorm fold
 *  bit 23 GroupNorm always in its two-launch form
 *  bits 24 - 26 shared-probability units of the self-attention launches (rt_op_attention_units_plan's mode)
 *  bit 27 GEGLU launches that cannot take the W-stationary order run groups of 8 tile rows
 *  bit 28 under-filled 3x3 convs on the split-K implicit GEMM instead of the chunk-split patch kernel
 *  bit 29 no two-halves chunk split for the 32x32 maps                  bit 30 the split rule counts streams of < 128 rows as whole tiles */
int rt_op_gemm_debug(int flags);
/* Second word of A/B switches (bits 0 - 30 of the first are taken; its bit 31 stays unused).  The engine wrapper reads RTDIFF_DEBUG_FLAGS2
 * once at load; csrc/common.h (DebugBit2) names the bits.  0 = default.
 *  bit 0  Upsample2D's convolutions stay on the patch kernel (nine taps on the nearest-2x up-sampled map, the route of rounds 2 - 6)
 *         instead of running as four 2x2 phase convolutions of the low-resolution map on csrc/gemm16.hip */
int rt_op_gemm_debug2(int flags);
/* Upsample2D (models/resnet.py: F.interpolate(scale_factor=2, mode="nearest") followed by the 3x3 convolution) in its sub-pixel form: output
 * pixel (2y + a, 2x + b) reads the 2x2 input pixels (y + a - 1 + r, x + b - 1 + c) only, with weights that are sums of the 3x3 taps.
 * rt_op_pack_upconv: w [Cout, Cin, 3, 3] (dtype RT_DTYPE_*) -> out_bf16 [phase 2a + b][Cout][tap 2r + c][Cin], summed in fp32 from the
 *   source values and rounded once (what rt_bind_weight stores next to the 3x3 pack of every `upsamplers.0.conv.weight`).
 * rt_op_upconv: rt_op_gemm mode 3 / epi 4 with the phase pack next to the 3x3 pack, as the engine's up-samplers pass it.  x bf16 NHWC [B, Hin, Win, Cin]; w9 bf16 [N, 9 Cin] (K index = tap * Cin + c, as
 *   rt_op_gemm mode 3); w_phase = rt_op_pack_upconv's output or NULL; out fp16 [B, 2 Hin, 2 Win, N].  *phase_route (may be NULL) = 1 when
 *   the four-phase launch runs (w_phase given, Cin % 64 == 0, the 16x16x32 family has a tile for ONE image's low-resolution map, switch
 *   clear), 0: the patch-kernel route of rt_op_gemm mode 3, bit for bit. */
int rt_op_pack_upconv(const void* w, int dtype, int Cout, int Cin, void* out_bf16, void* stream);
int rt_op_upconv(const void* x, const void* w9, const void* w_phase, const float* bias, void* out_f16, int B, int Hin, int Win, int Cin, int N,
                 int* phase_route, void* stream);

/* ---- VAE decoder: colour guidance (rd.py:151-168, xl.py:849-867) and plain decode (rd.py:227-236) ----
 * AutoencoderKL.decoder + post_quant_conv (diffusers 0.18.2, third party: architecture restated in oracle/vae.py).
 * Weight names are the AutoencoderKL state_dict keys ("decoder.conv_in.weight", "post_quant_conv.bias", ...). */
typedef struct rt_vae_config {
    int n_blocks;                         /* len(block_out_channels) */
    int block_out_channels[RT_MAX_LEVELS];
    int layers_per_block;                 /* decoder uses layers_per_block + 1 resnets per up block */
    int norm_groups;
    float scaling_factor;                 /* 0.18215 (SD) / 0.13025 (SDXL) */
    int latent_h, latent_w;               /* largest latent the workspace is sized for */
    int precise;                          /* 1: fp32-class contractions (operands as bf16 hi + lo pairs, three MFMA passes): what the SDXL
                                           * pipeline of the reference asks for (xl.py:856 decodes in fp32); 0: one bf16 pass */
} rt_vae_config;
typedef struct rt_vae rt_vae;
int rt_vae_create(const rt_vae_config* cfg, int device, rt_vae** out);
int rt_vae_destroy(rt_vae* v);
const char* rt_vae_last_error(rt_vae* v);
int rt_vae_weight_count(rt_vae* v);
int rt_vae_weight_info(rt_vae* v, int idx, char* name, int name_cap, int64_t* shape4, int* ndim);
int rt_vae_bind_weight(rt_vae* v, const char* name, const void* dev_ptr, int dtype, const int64_t* shape, int ndim);
int rt_vae_synchronize(rt_vae* v);
/* packed decoder weights (forward + backward-data copies), for the start-up broadcast next to rt_arena_info */
int rt_vae_arena_info(rt_vae* v, void** dev_ptr, uint64_t* bytes);
int rt_vae_arena_mark_bound(rt_vae* v);
/* img_out [3, 8h, 8w] f32 in [-1,1] = decode(latents [4,h,w] / scaling_factor if divide_by_scaling) */
int rt_vae_decode(rt_vae* v, const float* latents, int h, int w, int divide_by_scaling, float* img_out);
/* one guidance update, in place on `latents` [4,h,w]:
 *   x0 = (latents - noise_pred*sqrt(1-alpha_t))/sqrt(alpha_t); img = clamp(decode(x0/scaling)/2+.5, 0, 1)
 *   L = sum_k 100 * mse(sum(img*m_k)/sum(m_k), target_k);  latents -= dL/dlatents * weight * mask_all
 * masks_img [n, 8h*8w] (channel 0 of text_format_dict['color_obj_atten']), target_rgb_host [n*3],
 * mask_all [4,h,w] (text_format_dict['color_obj_atten_all']); grad_out [4,h,w] / loss_out_host optional. */
int rt_vae_color_guidance(rt_vae* v, float* latents, const float* noise_pred, float alpha_t, int h, int w, const float* masks_img,
                          const float* target_rgb_host, int n_regions, float weight, const float* mask_all, float* grad_out,
                          float* loss_out_host);

/* ---- VAE encoder: RegionDiffusion.encode_imgs (rd.py:238-246) ----
 * AutoencoderKL.encoder + quant_conv + DiagonalGaussianDistribution (diffusers 0.18.2, restated in tests/vae_encoder_ref.py; parity
 * unpinned against diffusers).  The same rt_vae handle type in the encoder role: weight names "encoder.*" / "quant_conv.*"; the
 * weight-table, bind, arena, synchronize, destroy and last-error calls serve both roles.  latent_h / latent_w of the config size the
 * workspace for images up to 8 latent_h x 8 latent_w.  Decode / guidance on an encoder handle and encode / sample on a decoder
 * handle return RT_E_STATE. */
int rt_vae_encoder_create(const rt_vae_config* cfg, int device, rt_vae** out);   /* device -1: weight table only */
/* img [3,H,W] f32 (H, W multiples of 8, at most the plan's), x' = in_scale*x + in_shift;
 * moments_out [8,H/8,W/8] = mean | clamp(logvar,-30,20) */
int rt_vae_encode(rt_vae* v, const float* img, int H, int W, float in_scale, float in_shift, float* moments_out);
/* latents [4,h,w] = scale * (mean + exp(0.5*logvar) * noise[4,h,w]) */
int rt_vae_posterior_sample(rt_vae* v, const float* moments, const float* noise, int h, int w, float scale, float* latents_out);

/* engine sampler state pointers for the guidance step: latents [4,h,w] and the CFG-combined noise prediction of the
 * last rt_region_step (noise_pred in rd.py:131-132 / xl.py:824-825) */
int rt_get_state_ptrs(rt_engine* e, float** latents, float** noise_pred);

#ifdef __cplusplus
}
#endif
#endif
