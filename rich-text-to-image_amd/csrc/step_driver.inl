// Host step drivers (included by engine.hip).  Flag logic follows the reference loops line by line:
//   SD  : models/region_diffusion.py:99-173        XL : models/region_diffusion_sdxl.py:779-872

static void pndm_coeffs(rt_engine* e, int i, SolverArgs& a) {
    // PNDMScheduler.step_plms (diffusers 0.18.2, [memory]); see oracle/schedulers.py:OraclePNDM
    SolverState& st = e->solver;
    const int ratio = 1000 / e->num_inference_steps;
    int t = (int)e->timesteps[i];
    int prev_t = t - ratio;
    a.push = 0;
    if (st.pndm_counter != 1) {
        a.push = 1;
        if (st.pndm_nets < 4) st.pndm_nets++;
        st.pndm_head = (st.pndm_head + 3) & 3;        // new newest slot
    } else {
        prev_t = t; t = t + ratio;
    }
    const size_t per = (size_t)2 * 4 * e->lat_h * e->lat_w;
    for (int k = 0; k < 4; ++k) a.ets[k] = e->ets + (size_t)((st.pndm_head + k) & 3) * per;
    if (!a.push) { for (int k = 3; k >= 1; --k) a.ets[k] = a.ets[k - 1]; }   // ets[1] = newest stored
    if (st.pndm_nets == 1 && st.pndm_counter == 0) a.pndm_mode = 0;
    else if (st.pndm_nets == 1 && st.pndm_counter == 1) a.pndm_mode = 1;
    else a.pndm_mode = st.pndm_nets;   // 2, 3, 4
    RT_REQUIRE((int)e->table.size() >= 1000, "pndm: alphas_cumprod table missing");
    const double a_t = e->table[t], a_p = prev_t >= 0 ? e->table[prev_t] : e->table[0];
    const double b_t = 1 - a_t, b_p = 1 - a_p;
    // computed in fp32 like the reference's tensor arithmetic on fp32 alphas
    const float fa_t = (float)a_t, fa_p = (float)a_p, fb_t = (float)b_t, fb_p = (float)b_p;
    const float sample_coeff = std::sqrt(fa_p / fa_t);
    const float denom = fa_t * std::sqrt(fb_p) + std::sqrt(fa_t * fb_t * fa_p);
    a.ca = sample_coeff; a.cb = (fa_p - fa_t) / denom;
    a.cur_sample = e->cur_sample;
    st.pndm_counter++;
}

// What DPM-Solver++ and SDE-DPM-Solver++ share (DPMSolverMultistepScheduler, diffusers 0.18.2, [memory]: midpoint, epsilon,
// lower_order_final, no thresholding; see tests/dpm_solver_ref.py and tests/sde_ref.py).  fp32 scalars in diffusers' tensor order:
// alpha = sqrt(ac), sigma = sqrt(1 - ac), lambda = log(alpha) - log(sigma); s0 = t_i, s1 = t_{i-1}, p = t_{i+1} (0 after the last step).
// Fills alpha_s0, sigma_s0, order, inv_r0 and the history slots, advances the solver state; the callers add ratio / c1 / c2 (and cn).
struct MultistepPoint { float h, alpha_p, sigma_p; };
static MultistepPoint multistep_coeffs(rt_engine* e, int i, bool single_step, SolverArgs& d) {
    const std::string who = rt_sched_is_stoch(e->sched_kind) ? "sde-dpm-solver++" : "dpm-solver++";
    RT_REQUIRE((int)e->table.size() >= 1000, who + ": alphas_cumprod table missing");
    const int n = (int)e->timesteps.size();
    RT_REQUIRE(i >= 0 && i < n, who + ": step index out of range");
    SolverState& st = e->solver;
    auto alpha = [&](int t) { return std::sqrt(e->table[t]); };
    auto sigma = [&](int t) { return std::sqrt(1.f - e->table[t]); };
    auto lambda = [&](int t) { return std::log(alpha(t)) - std::log(sigma(t)); };
    const int s0 = (int)e->timesteps[i], p = i == n - 1 ? 0 : (int)e->timesteps[i + 1];
    const bool lower_order_final = i == n - 1 && n < 15;
    const bool first = single_step || st.dpm_lower_order_nums < 1 || lower_order_final || i == 0;
    const float h = lambda(p) - lambda(s0);
    d.alpha_s0 = alpha(s0); d.sigma_s0 = sigma(s0);
    d.order = first ? 1 : 2;
    d.inv_r0 = 0.f;
    if (!first) {
        const int s1 = (int)e->timesteps[i - 1];
        const float r0 = (lambda(s0) - lambda(s1)) / h;
        d.inv_r0 = 1.f / r0;
    }
    // two history slots per stream in the PNDM buffer ([slot][stream][4*HW]): this step writes x0 into one and reads m1 from the other.
    // A stream that is not stepped (the reference pair once it stops) leaves its half of both slots alone and is never stepped again.
    const size_t per = (size_t)2 * 4 * e->lat_h * e->lat_w;
    d.ets[0] = e->ets + (size_t)st.dpm_head * per;
    d.ets[1] = e->ets + (size_t)(st.dpm_head ^ 1) * per;
    st.dpm_head ^= 1;
    if (st.dpm_lower_order_nums < 2) st.dpm_lower_order_nums++;
    return {h, alpha(p), sigma(p)};
}

// The solver of sched_kind and its scalars of step i; fp32, evaluated left to right.
static void solver_coeffs(rt_engine* e, int i, SolverArgs& d) {
    const int kind = e->sched_kind;
    if (kind == RT_SCHED_PNDM) { d.solver = STEP_PLMS; pndm_coeffs(e, i, d); return; }
    if (kind == RT_SCHED_EULER) { d.solver = STEP_EULER; d.dsigma = e->table[i + 1] - e->table[i]; return; }
    if (rt_sched_is_stoch(kind)) {
        // the noise field of the step is a function of (noise_seed, i, pixel): csrc/philox.h
        RT_REQUIRE(i >= 0 && i < (int)e->timesteps.size(), "stochastic sampler: step index out of range");
        d.seed_lo = (unsigned)(e->noise_seed & 0xffffffffull); d.seed_hi = (unsigned)(e->noise_seed >> 32); d.step = i;
    }
    if (kind == RT_SCHED_EULER_A) {
        // EulerAncestralDiscreteScheduler: sigma_up = sqrt(s'^2 (s^2 - s'^2) / s^2), sigma_down = sqrt(s'^2 - sigma_up^2);
        // x' = x + eps (sigma_down - s) + z sigma_up.  The last step has s' = 0: no noise.
        const float sg = e->table[i], sp = e->table[i + 1];
        const float up = std::sqrt(sp * sp * (sg * sg - sp * sp) / (sg * sg));
        const float down = std::sqrt(sp * sp - up * up);
        d.solver = STEP_EULER_A; d.dsigma = down - sg; d.cn = up;
        return;
    }
    const bool sde = rt_sched_is_stoch(kind);
    const MultistepPoint m = multistep_coeffs(e, i, kind == RT_SCHED_DPMPP_1 || kind == RT_SCHED_DPMPP_SDE_1, d);
    if (!sde) {
        d.solver = STEP_DPM;
        d.ratio = m.sigma_p / d.sigma_s0;
        d.c1 = m.alpha_p * (std::exp(-m.h) - 1.f);
    } else {
        //   x' = (sigma_p / sigma_s0 exp(-h)) x + alpha_p (1 - exp(-2h)) x0 [+ 0.5 alpha_p (1 - exp(-2h)) (1 / r0) (x0 - m1)] + sigma_p sqrt(1 - exp(-2h)) z
        const float q = 1.f - std::exp(-2.f * m.h);
        d.solver = STEP_SDE;
        d.ratio = m.sigma_p / d.sigma_s0 * std::exp(-m.h);
        d.c1 = m.alpha_p * q;
        d.cn = m.sigma_p * std::sqrt(q);
    }
    d.c2 = 0.5f * d.c1;
}

// The streams of rich-text step i and the flags of its epilogue (everything of region_step that is a pure function of the schedule
// position): `in` = the F batched forwards with their mode words, `a` = the epilogue's arguments without the scheduler coefficients
// (PNDM's are stateful: finish_step computes them once).
void rt_engine::region_plan(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend, FwdIn& in, StepArgs& a, bool& blend_out,
                            bool& inject_out) {
    require_bound();
    const int n = (int)timesteps.size(), R = n_regions;
    RT_REQUIRE(i >= 0 && i < n, "region_step: step index out of range");
    RT_REQUIRE(R >= 1 && n_prompts == R + 1, "region_step: need R masks and R+1 prompts (rd.py:96-97)");
    RT_REQUIRE(mask_hw == lat_h * lat_w && lat_h > 0, "region_step: masks/latents shape mismatch");
    RT_REQUIRE(rt_sched_is_dpm(sched_kind) || rt_sched_is_euler(sched_kind) == xl,
               "region_step: SD uses PNDM or DPM-Solver++, SDXL uses Euler or DPM-Solver++");
    pag_step_check(g);
    const float t = timesteps[i];
    const bool use_ref = isa > 0 || ibg > 0;
    // `t > (1-inject_selfattn)*1000`: torch compares a float32 / int64 tensor element with a Python float in float32
    const float thr = (float)((1.0 - isa) * 1000.0);
    auto feat_at = [&](int j) { return timesteps[j] > thr; };
    const bool feat = feat_at(i);
    const int bg_index = (int)(ibg * (double)n);                   // int(inject_background * len(timesteps)) on Python floats
    const bool blend = (i == bg_index) && ibg > 0;
    bool step_ref = use_ref;
    if (xl) step_ref = isa > 0 || ((double)i < ibg * (double)n);
    bool run_ref = use_ref;
    if (use_ref && elide) {
        // the reference pair can only influence the output through injection at this step, or through
        // latents_reference consumed by a later injected step or by the blend
        int last_use = ibg > 0 ? bg_index : -1;
        for (int j = 0; j < n; ++j) if (feat_at(j)) last_use = std::max(last_use, j);
        run_ref = i <= last_use;
    }
    if (!run_ref) step_ref = false;

    in = FwdIn{}; in.h = lat_h; in.w = lat_w; in.t = t; in.eps_out = eps;
    const float scale = rt_sched_is_euler(sched_kind) ? 1.f / std::sqrt(table[i] * table[i] + 1.f) : 1.f;   // Euler's scale_model_input
    a = StepArgs{};
    int F = 0;
    auto add = [&](const float* x, int prompt, int fs) {
        RT_REQUIRE(F < cfg.max_streams, "region_step: more streams than max_streams");
        in.x[F] = x; in.scale[F] = scale; in.prompt[F] = prompt; in.fontsize[F] = fs; in.qk_src[F] = F; in.res_src[F] = -1;
        return F++;
    };
    a.s_uncond = add(lat, 0, 0);
    a.s_base = add(lat, R, 1);
    a.s_uref = a.s_tref = -1;
    if (run_ref) { a.s_uref = add(lat_ref, 0, 0); a.s_tref = add(lat_ref, R, 0); }
    for (int r = 0; r < R - 1; ++r) {
        const int s = add(lat, r + 1, 0);
        if (feat && run_ref) { in.qk_src[s] = a.s_tref; in.res_src[s] = a.s_tref; }
        a.s_region[r] = s;
    }
    // Perturbed-attention guidance: the twins behind all existing streams - of base, of text_ref while the pair is stepped (the plain pass's
    // treatment, with the base slot's sigma), of the region streams whose slot has sigma != 0 - and the pairs of the step's fold
    pag_pairs = PagPairs{};
    if (pag_on()) {
        auto pair = [&](int s, float sigma) {
            PagPairs& p = pag_pairs;
            p.s[p.n] = s; p.twin[p.n] = pag_twin(in, F, s, "region_step"); p.rho[p.n] = sigma / g; ++p.n;
        };
        if (pag_scale[R] != 0.f) {
            pair(a.s_base, pag_scale[R]);
            if (step_ref) pair(a.s_tref, pag_scale[R]);
        }
        for (int r = 0; r < R - 1; ++r) if (pag_scale[r + 1] != 0.f) pair(a.s_region[r], pag_scale[r + 1]);
    }
    in.B = F; pag_pairs.F = F;
    a.eps = eps; a.masks = masks; a.lat = lat; a.lat_ref = lat_ref; a.HW = lat_h * lat_w; a.R = R; a.g = g; a.plain = 0;
    a.noise_pred = noise_pred;
    a.step_ref = step_ref ? 1 : 0; a.blend = (blend && !defer_blend) ? 1 : 0;
    blend_out = blend && defer_blend;
    inject_out = feat && run_ref;
}

// The guided-prediction pre-pass (guided.hip) of step i, when the model predicts v or the guidance is rescaled: composes the guided
// prediction of the main stream and of the stepped reference pair into `gpred`, rescales it, converts v to the epsilon-equivalent at the
// point where the UNet was evaluated, and re-aims the epilogue's arguments at `gpred` as a plain two-stream buffer whose unconditional
// and text slots coincide (E + g (E - E) = E).  R, masks, blend, step_ref and noise_pred stay as planned.  fp32 scalars, left to right:
//   sigma space (Euler, Euler ancestral):          cv = 1 / sqrt(sigma_i^2 + 1),  cx = sigma_i / (sigma_i^2 + 1)
//   VP (PNDM, DPM-Solver++, SDE-DPM-Solver++):      cv = sqrt(ac_t),  cx = sqrt(1 - ac_t),  t = timesteps[i] (PNDM's repeated one as listed)
// [memory] diffusers' PNDM converts v after the multistep combination, with the current sample; here the history holds
// epsilon-equivalents - the epsilon-model the v-model defines - so the five solvers stay untouched.
void rt_engine::guided_prepass(int i, StepArgs& a) {
    GuidedArgs q{};
    q.s = a; q.gpred = gpred; q.partials = gpartials; q.factors = gfactors;
    q.phi = guidance_rescale; q.vpred = prediction_type == RT_PRED_V ? 1 : 0;
    if (q.vpred) {
        if (rt_sched_is_euler(sched_kind)) {
            const float sg = table[i];
            q.cv = 1.f / std::sqrt(sg * sg + 1.f); q.cx = sg / (sg * sg + 1.f);
        } else {
            RT_REQUIRE((int)table.size() >= 1000, "v-prediction: alphas_cumprod table missing");
            const int t = (int)timesteps[i];
            RT_REQUIRE(t >= 0 && t < (int)table.size(), "v-prediction: timestep outside the table");
            q.cv = std::sqrt(table[t]); q.cx = std::sqrt(1.f - table[t]);
        }
    }
    launch_guided_prediction(q, stream);
    const bool has_ref = a.s_uref >= 0 && a.step_ref;
    a.eps = gpred; a.plain = 1; a.s_uncond = a.s_base = 0; a.s_uref = a.s_tref = has_ref ? 1 : -1;
}

// The epilogue of step i on the planned arguments: the guided pre-pass when the prediction needs it, then the solver of sched_kind
void rt_engine::finish_step(int i, StepArgs& a) {
    pag_fold();      // perturbed-attention guidance: after it the two-term guidance below is the three-term one
    if (prediction_type != RT_PRED_EPSILON || guidance_rescale > 0.f) guided_prepass(i, a);
    SolverArgs d{};
    solver_coeffs(this, i, d);
    launch_step_epilogue(a, d, stream);
    solver.steps_done++;
}

// mask combine + CFG + scheduler step + blend on the eps of ALL streams of step i (models/region_diffusion.py:119-147,
// region_diffusion_sdxl.py:810-846)
void rt_engine::region_finish(int i, StepArgs& a, bool blend_deferred) {
    pending_blend = blend_deferred;
    finish_step(i, a);
}

void rt_engine::region_step(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend) {
    FwdIn in; StepArgs a; bool blend_deferred, inject;
    region_plan(i, g, isa, ibg, xl, elide, defer_blend, in, a, blend_deferred, inject);
    unet_forward(in);
    region_finish(i, a, blend_deferred);
}

// ---- intra-image split of a step over `nparts` GPUs.  The F forwards of a step are independent except that the
// region streams of an injected step consume the self-attention Q / K and one ResNet feature of the text_ref stream, layer by layer
// (0.42 GB per step if shipped).  The streams are therefore cut into `nparts` CONTIGUOUS ranges of the step's stream list
// [uncond, base, uncond_ref, text_ref, region 0 ..] such that text_ref and every region stream land in the same (the last) range: no
// per-layer traffic at all, ONE exchange of the noise predictions (F x 4 x h x w fp32: 1.8 MB at SDXL) per step, after which every
// rank runs the (elementwise) epilogue on the full set and holds identical latents.  With 2 parts: {uncond, base, uncond_ref} |
// {text_ref, regions} while the injection is on, halves otherwise.  Batch invariance (a stream's forward does not depend on the
// other streams of its launch) makes the split run bit-identical with the one-GPU step.
static void region_split_range(int F, int s_tref, bool inject, int part, int nparts, int* first, int* count) {
    RT_REQUIRE(nparts >= 1 && part >= 0 && part < nparts && F >= 1, "split: part index");
    // even prefix split of the stream list; while the injection is on, everything from text_ref on forms the LAST part and the streams
    // before it (uncond, base, uncond_ref: independent forwards) are dealt evenly to the other parts
    int lo, hi;
    if (inject && s_tref >= 0 && nparts > 1) {
        const int head = s_tref, np = nparts - 1;
        auto bound = [&](int k) { return (int)(((long)head * k + np - 1) / np); };       // ceil(head k / (nparts - 1))
        if (part == nparts - 1) { lo = head; hi = F; } else { lo = bound(part); hi = bound(part + 1); }
    } else {
        auto bound = [&](int k) { return (int)(((long)F * k + nparts - 1) / nparts); };   // ceil(F k / nparts)
        lo = bound(part); hi = bound(part + 1);
    }
    *first = lo; *count = hi > lo ? hi - lo : 0;
}

void rt_engine::region_step_part(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend, int part, int nparts, int* first,
                                 int* count, int* plan_info) {
    FwdIn in; StepArgs a; bool blend_deferred, inject;
    region_plan(i, g, isa, ibg, xl, elide, defer_blend, in, a, blend_deferred, inject);
    region_split_range(in.B, a.s_tref, inject, part, nparts, first, count);
    if (plan_info) { plan_info[0] = in.B; plan_info[1] = a.s_tref; plan_info[2] = inject ? 1 : 0; }      // what rt_op_split_range needs for the other parts' ranges
    if (*count == 0) return;
    FwdIn sub{}; sub.h = in.h; sub.w = in.w; sub.t = in.t; sub.B = *count;
    sub.eps_out = eps + (size_t)*first * lat_h * lat_w * 4;          // the range is contiguous: its predictions land in their own slots
    for (int b = 0; b < *count; ++b) {
        const int s = *first + b;
        sub.x[b] = in.x[s]; sub.scale[b] = in.scale[s]; sub.prompt[b] = in.prompt[s]; sub.fontsize[b] = in.fontsize[s]; sub.perturb[b] = in.perturb[s];
        RT_REQUIRE(in.qk_src[s] >= *first && in.qk_src[s] < *first + *count, "split: a stream's Q / K source lies outside its part");
        sub.qk_src[b] = in.qk_src[s] - *first;
        sub.res_src[b] = in.res_src[s] < 0 ? -1 : in.res_src[s] - *first;
    }
    unet_forward(sub);
}

void rt_engine::region_step_finish(int i, float g, double isa, double ibg, bool xl, bool elide, bool defer_blend) {
    FwdIn in; StepArgs a; bool blend_deferred, inject;
    region_plan(i, g, isa, ibg, xl, elide, defer_blend, in, a, blend_deferred, inject);
    region_finish(i, a, blend_deferred);
}

// The plain-text step (rd.py:200-214 / xl.py:880-905) in the same three pieces as the rich-text step: the forwards of a contiguous range of
// its two streams [uncond, text], and the epilogue on both.  `first < 0`: both streams (the one-GPU step).
// Perturbed-attention guidance (the text slot's sigma != 0) appends the twin of the text stream: [uncond, text, twin].
int rt_engine::plain_streams() {
    if (!pag_on()) return 2;
    RT_REQUIRE(n_prompts >= 2, "plain_step: need [negative, text] prompts");
    if (pag_scale[1] == 0.f) return 2;
    if (cfg.max_streams < 3)
        throw rt_error(RT_E_INVALID, "plain_step: perturbed-attention guidance needs more streams (3) than the engine was built for (max_streams " +
                                         std::to_string(cfg.max_streams) + ")");
    return 3;
}
void rt_engine::plain_forward(int i, int first, int count) {
    require_bound();
    const int n = (int)timesteps.size();
    RT_REQUIRE(i >= 0 && i < n, "plain_step: step index out of range");
    RT_REQUIRE(n_prompts >= 2, "plain_step: need [negative, text] prompts");
    RT_REQUIRE(first >= 0 && count >= 1 && first + count <= plain_streams(), "plain_step: stream range");
    // perturbed-attention guidance: what can be refused without g is refused here, before any launch of the split form too (rt_plain_step_part
    // has no g: g == 0 is caught by rt_plain_step_finish, ahead of its own launches; rt_plain_step checks both first)
    pag_step_check(1.f);
    const bool xl = rt_sched_is_euler(sched_kind);
    FwdIn in{}; in.h = lat_h; in.w = lat_w; in.t = timesteps[i]; in.B = count;
    in.eps_out = eps + (size_t)first * lat_h * lat_w * 4;            // a stream's prediction lands in its own slot of the eps buffer
    const float scale = xl ? 1.f / std::sqrt(table[i] * table[i] + 1.f) : 1.f;
    for (int b = 0; b < count; ++b) {
        const int s = first + b;                                        // stream 2: the twin of the text stream
        in.x[b] = lat; in.scale[b] = scale; in.prompt[b] = s < 2 ? s : 1; in.fontsize[b] = 0; in.qk_src[b] = b; in.res_src[b] = -1; in.perturb[b] = s == 2;
    }
    // hooks keep the conditional half: out[1][0][1:2] (rd.py:417,425 / xl.py:980,991) - recorded by the rank that runs the text stream
    if (any_store() && first <= 1 && first + count > 1) in.store_stream = 1 - first;
    unet_forward(in);
}
void rt_engine::plain_finish(int i, float g) {
    RT_REQUIRE(i >= 0 && i < (int)timesteps.size(), "plain_step: step index out of range");     // PNDM / Euler index their tables with it
    pag_step_check(g);
    pag_pairs = PagPairs{};
    if (plain_streams() == 3) { pag_pairs.n = 1; pag_pairs.F = 3; pag_pairs.s[0] = 1; pag_pairs.twin[0] = 2; pag_pairs.rho[0] = pag_scale[1] / g; }
    StepArgs a{};
    a.eps = eps; a.masks = masks; a.lat = lat; a.lat_ref = lat_ref; a.HW = lat_h * lat_w; a.R = 0; a.g = g; a.plain = 1;
    a.s_uncond = 0; a.s_base = 1; a.s_uref = a.s_tref = -1; a.step_ref = 0; a.blend = 0;
    finish_step(i, a);
}
void rt_engine::plain_step(int i, float g) {
    pag_step_check(g);
    plain_forward(i, 0, plain_streams());
    plain_finish(i, g);
}
// Intra-image split of the plain pass (round 6): part 0 runs the unconditional stream, part 1 the text stream (and records the token maps),
// further parts run nothing; one exchange of the two noise predictions, then rt_plain_step_finish on every rank.
void rt_engine::plain_step_part(int i, int part, int nparts, int* first, int* count) {
    RT_REQUIRE(nparts >= 1 && part >= 0 && part < nparts, "plain_step_part: part index");
    // (with perturbed-attention guidance the twin rides with the text stream's part)
    const int F = plain_streams();
    if (nparts == 1) { *first = 0; *count = F; }
    else { *first = part < 2 ? part : F; *count = part == 0 ? 1 : part == 1 ? F - 1 : 0; }
    if (*count > 0) plain_forward(i, *first, *count);
    else { require_bound(); RT_REQUIRE(i >= 0 && i < (int)timesteps.size(), "plain_step: step index out of range"); }
}
