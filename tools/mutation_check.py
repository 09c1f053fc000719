#!/usr/bin/env python3
"""Do the tests notice a known bug?  Puts the terminal-observation bugs that lived in the kernels through rounds 1-5 back into
a COPY of csrc/ (the fixes were commits b1ce333 and 8b54a4a, and round 6's log_plane fix), builds it, and runs the round-6 coverage
tests against the mutant: every mutant must be caught ("What's weak" 2 / "Next round" 1).  The learner mutants
(the PPO update, fwgym_learner.h) are plausible slips of a rewrite of its kernels; they run the emulated forms of
tests/test_ppo_hip_contract.py (the ppo_cnn_* ones, slips in the backward pass through the CNN learner's conv, those of
tests/test_ppo_hip_cnn.py).  The head mutants (head_*: the rollout head, fwgym_actor.h) likewise, against the emulated forms of
tests/test_actor_contract.py (the head_cnn_* ones, slips in the CNN head's own code, those of tests/test_actor_contract_cnn.py); they are
built for the host emulation only.  The eval_* mutants (the evaluation protocol on the device,
fwgym_eval.h) run tests/test_eval_device.py; the recorder_* mutants (the device flight recorder, fwgym_record.h) tests/test_recorder.py;
the monitor_* mutants (the device training monitor, fwgym_monitor.h) the kernel tests of tests/test_monitor.py; the goal_* mutants
(the goal env, fwgym_goal.h) the kernel tests of tests/test_goal.py; the replay_* mutants (the hindsight replay buffer, fwgym_replay.h)
the kernel tests of tests/test_replay.py; the ddpg_* mutants (the off-policy update, fwgym_offpolicy.h) the emulated forms of
tests/test_offpolicy_contract.py; the behaviour_* mutants (the behaviour head, fwgym_behaviour.h) the emulated forms of
tests/test_behaviour.py.

    python tools/mutation_check.py emu [NAME ...]     # host emulation: each mutant (or the NAMEd) against its own tests (TESTS)
    python tools/mutation_check.py hip OUTDIR          # gfx950 libraries of the mutants (tools/devlib.py), for a GPU session:
                                                       # FWGYM_MUTANT_LIB_ROW_LOG=... python -m pytest tests/test_gpu_oracle_coverage.py

Never the product: the mutated sources live in a temporary directory."""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fixed-wing-gym_amd", "csrc")

MUTANTS = {
    # b1ce333 reverted: after a FAILED step under turbulence the air data are re-derived with the failed step's gust
    "airdata": [("fwgym.hip", """                if (TURB) {   // (air data: as the last committed step left them -- derived with its gust, see store_sim)
                    const float4 q = CGROUP(A.S, A.N, (c.L.derived >> 2) + 1, e);
                    E.d.alpha = q.x; E.d.beta = q.y; E.d.Va = q.z;
                }
""", "")],
    # 8b54a4a reverted: a foreseen end whose last step fails is installed by the physics wave all the same in the dense layout
    # (only the row log's partner_rows rule holds it back)
    "install_on_failed_last_step": [
        ("fwgym.hip", "        if (pre_install) pre_rows = pre_rows && fail == 0;", "        if (partner_rows) pre_rows = pre_rows && fail == 0;"),
        ("fwgym.hip", "            end_p = pre_install && valid && f2u(w.z) != 0u && fail == 0;",
         "            end_p = pre_install && valid && f2u(w.z) != 0u && !(partner_rows && fail != 0);")],
    # round 6's own find reverted (log_plane: a record one further back than the carried rows is at its home plane): the oldest
    # row of a failed step's terminal observation on the row log's wrap step, obs_step 1 (the shipped cnn configuration)
    "log_plane_past_the_log": [
        ("fwgym_env.h", "    return (long long)p * L + home + ((wraps > 0 && home <= len - 2) ? (long long)P * wraps : 0);",
         "    return (long long)p * L + home + (long long)P * wraps;")],
    # the PPO update: the minibatch's rows read in buffer order instead of through the permutation
    "ppo_gather_ignores_idx": [
        ("fwgym_learner.h", "            const long long row = ok ? G.idx[r0 + r] : 0;",
         "            const long long row = ok ? (long long)(r0 + r) : 0;")],
    # the rows of a tail tile past the minibatch counted in the loss terms
    "ppo_loss_tail_unmasked": [
        ("fwgym_learner.h", "                const bool ok = r < nrows;\n                const float* rf = rowf + r * 8;",
         "                const bool ok = true;\n                const float* rf = rowf + r * 8;")],
    # the last workgroup's partial gradient left out of the sum
    "ppo_reduce_drops_a_slab": [
        ("fwgym_learner.h", "    for (int b = 0; b < nslab; ++b) s += slab[(size_t)b * L.SW + j];",
         "    for (int b = 0; b < nslab - 1; ++b) s += slab[(size_t)b * L.SW + j];")],
    # the advantages normalised by the unbiased std (PPO2 and ppo_loss take the biased one)
    "ppo_moments_unbiased_std": [
        ("fwgym_learner.h", "        mom[2 * blockIdx.x + 1] = (float)sqrt(red[0] / (double)mb) + 1e-8f;",
         "        mom[2 * blockIdx.x + 1] = (float)sqrt(red[0] / (double)(mb - 1)) + 1e-8f;")],
    # the head repacked on the device without the low bf16 parts of the weights
    "actor_pack_zero_low_parts": [
        ("fwgym_learner.h", "        frags[((net * 2 + 1) * nfw + f) * 64 + l] = frag_t{wl[0], wl[1], wl[2], wl[3]};",
         "        frags[((net * 2 + 1) * nfw + f) * 64 + l] = frag_t{0u, 0u, 0u, 0u};")],
    # the CNN learner (k_ppo_grad<true>): the value network's term left out of dL / d(conv output) -- the conv is shared by pi and vf
    "ppo_cnn_dc_drops_vf": [
        ("fwgym_learner.h", "                ppo_mma_tile<CNN>(dc, Tb, LS, 1, tm0, 64, W1, FWG_CNN_K, 1, tn0, FWG_CNN_K, 64, 64, l);",
         "                if (net == 0) ppo_mma_tile<CNN>(dc, Tb, LS, 1, tm0, 64, W1, FWG_CNN_K, 1, tn0, FWG_CNN_K, 64, 64, l);")],
    # the conv's bias gradient summed over one of the 12 features only
    "ppo_cnn_conv_bias_one_feature": [
        ("fwgym_learner.h", "                    for (int j = 0; j < FWG_CNN_COLS; ++j)\n",
         "                    for (int j = 0; j < (isw ? FWG_CNN_COLS : 1); ++j)\n")],
    # ---- the tag (configuration generation, episode) on prepared reset draws: what keeps a draw of the old ranges out after
    # set_curriculum_level.  The generation dropped from the two waves' decision whether a complete draw is used / installed
    "draw_ready_ignores_generation": [
        ("fwgym.hip", "        if (pre_install) pre_rows = pre_draw && f2u(pre_tag.x) == dc.generation && f2u(pre_tag.y) == E.episode + 1u;",
         "        if (pre_install) pre_rows = pre_draw && f2u(pre_tag.y) == E.episode + 1u;"),
        ("fwgym.hip", "                ready = pre_draw && f2u(pre_tag.x) == dc.generation && f2u(pre_tag.y) == E.episode + 1u;",
         "                ready = pre_draw && f2u(pre_tag.y) == E.episode + 1u;")],
    # ... from the check that discards the pieces of a half-prepared draw
    "draw_piece_ignores_generation": [
        ("fwgym_env.h", "        if (f2u(tag.x) != dc.generation || f2u(tag.y) != episode_new) stage = 0u;",
         "        if (f2u(tag.y) != episode_new) stage = 0u;")],
    # ... from the tags of the per-env aircraft constants and reward scalings (k_model_draw, k_model_draw_q)
    "model_draw_ignores_generation": [
        ("fwgym.hip", "        if (!(f2u(tag.x) == episode_new && f2u(tag.y) == dp->generation)) {", "        if (!(f2u(tag.x) == episode_new)) {"),
        ("fwgym.hip", "    if (f2u(tag.y) == episode_new && f2u(tag.z) == dp->generation) return;", "    if (f2u(tag.y) == episode_new) return;"),
        ("fwgym.hip", "        if (f2u(tag.y) == episode_new && f2u(tag.z) == dp->generation) continue;   // (wave-uniform)",
         "        if (f2u(tag.y) == episode_new) continue;   // (wave-uniform)")],
    # fwg_update_config leaves the generation where it is
    "update_config_keeps_generation": [
        ("fwgym.hip", "    dy.generation = h->hd.generation + 1u;   // ranges may have changed: prepared reset draws are stale",
         "    dy.generation = h->hd.generation;")],
    # ---- the rollout head (fwgym_actor.h), arithmetic only and in bounds: plausible slips of a rewrite for speed; they run the
    # emulated forms of tests/test_actor_contract.py.  One of the three split-bf16 products (A_lo B_hi) dropped: from mma3 and
    # from the two forms of it the head's networks go through (mma3x2: layers 1 and 2, mma3s: layer 3; mma3 itself serves the learner)
    "head_split_drops_a_lo_product": [
        ("fwgym_actor.h", "        acc = fwg_mfma_bf16(a_lo, b_hi, acc);\n", ""),
        ("fwgym_actor.h", "        acc0 = fwg_mfma_bf16(a0_lo, b_hi, acc0); acc1 = fwg_mfma_bf16(a1_lo, b_hi, acc1);\n", ""),
        ("fwgym_actor.h", "        acc_a = fwg_mfma_bf16(a_lo, b_hi, acc_a);\n", "")],
    # the observation fold without the term for the distance between the batch mean and the running mean
    "head_fold_drops_delta_term": [
        ("fwgym_actor.h", "const float mm = v * cnt + bvar * n_obs + s1 * s1 * (cnt * n_obs / tt);", "const float mm = v * cnt + bvar * n_obs;")],
    # the discounted return carried over an episode end
    "head_return_ignores_done": [
        ("fwgym_actor.h", "        A.ret[e] = (A.done != nullptr && A.done[e]) ? 0.f : r;", "        A.ret[e] = r;")],
    # the sampling noise drawn for env ids that start at 0 whatever env_id_base says
    "head_noise_ignores_env_base": [
        ("fwgym_actor.h", "philox4x32((unsigned)(A.env_base + e), act_ctr,", "philox4x32((unsigned)(e), act_ctr,")],
    # the scalar load path (obs_dim % 4 != 0) one feature short
    "head_scalar_load_one_short": [
        ("fwgym_actor.h", "if (f0 + i < A.D) v[i] = A.obs[e * A.D + f0 + i];", "if (f0 + i + 1 < A.D) v[i] = A.obs[e * A.D + f0 + i];")],
    # the act counter (the noise stream's counter, and the rotation of the accumulator sets) kept by deterministic acts
    "head_counter_skips_deterministic_acts": [
        ("fwgym_actor.h", "                S1.act_counter = act_ctr + 1u;", "                S1.act_counter = act_ctr + (A.deterministic ? 0u : 1u);")],
    # ---- the CNN rollout head (actor_block<SPLIT, 3, true> and its launch), arithmetic only and in bounds; they run the emulated
    # forms of tests/test_actor_contract_cnn.py.  Every filter's conv output takes filter 0's bias
    "head_cnn_bias_of_filter_0": [
        ("fwgym_actor.h", "            float z = cnn_p[FWG_CNN_ROWS * FWG_CNN_FILTERS + c];", "            float z = cnn_p[FWG_CNN_ROWS * FWG_CNN_FILTERS + 0];")],
    # the conv without the window's last row (the newest record)
    "head_cnn_conv_drops_last_row": [
        ("fwgym_actor.h", "for (int r = 0; r < FWG_CNN_ROWS; ++r) z = fmaf(", "for (int r = 0; r < FWG_CNN_ROWS - 1; ++r) z = fmaf(")],
    # the CNN branch's own normalisation line without the clip
    "head_cnn_no_obs_clip": [
        ("fwgym_actor.h", "xn[4 * q + i] = fminf(fmaxf((r4[i] - mean_s[4 * q + i]) * rstd_s[4 * q + i], -A.clip_obs), A.clip_obs);",
         "xn[4 * q + i] = (r4[i] - mean_s[4 * q + i]) * rstd_s[4 * q + i];")],
    # precise=False launches the split-bf16 instance all the same (its LDS request is the larger one: in bounds)
    "head_cnn_plain_launches_split": [
        ("fwgym.hip", "        if (a->precise) hipLaunchKernelGGL((k_actor_act_cnn<3>), grid, block, a->lds_cnn[1], st, A);\n"
                      "        else hipLaunchKernelGGL((k_actor_act_cnn<1>), grid, block, a->lds_cnn[0], st, A);\n",
         "        hipLaunchKernelGGL((k_actor_act_cnn<3>), grid, block, a->lds_cnn[1], st, A);\n")],
    # on a row log every row of the window read from the window's first plane (the dense batch is read as before)
    "head_cnn_log_window_one_plane": [
        ("fwgym_actor.h", "    return A.obs + ((win + r) * A.N + e) * A.obs_n + j;", "    return A.obs + (win * A.N + e) * A.obs_n + j;")],
    # ---- the evaluation protocol on the device (fwgym_eval.h); they run the emulated forms, tests/test_eval_device.py.
    # The tracker latches every done, not the first: metrics_final and termination overwritten when a finished env reports done again
    "eval_tracker_latches_every_done": [
        ("fwgym_eval.h", "    if (t > 0) {\n        if (on) {\n", "    if (t > 0) {\n        if (!on && done[e]) {\n"
         "            termination[e] = term[e];\n            for (int k = 0; k < FWG_N_METRICS; ++k) metrics_final[k * N + e] = metrics[k * N + e];\n        }\n        if (on) {\n")],
    # the gate multiplies the action rows of finished envs by zero instead of storing zeros (0 * NaN = NaN reaches the step)
    "eval_gate_multiplies": [
        ("fwgym_eval.h", "{ actions[3 * e] = 0.f; actions[3 * e + 1] = 0.f; actions[3 * e + 2] = 0.f; }",
         "{ actions[3 * e] *= 0.f; actions[3 * e + 1] *= 0.f; actions[3 * e + 2] *= 0.f; }")],
    # the PID adds dt * e to the integrators BEFORE it computes the action
    "eval_pid_integrates_first": [
        ("fwgym_eval.h", "    const float i_phi = integ[e], i_theta = integ[N + e], i_va = integ[2 * N + e];",
         "    const float i_phi = integ[e] + g.dt * e_phi, i_theta = integ[N + e] + g.dt * e_theta, i_va = integ[2 * N + e] + g.dt * e_va;"),
        ("fwgym_eval.h", "    integ[e] = i_phi + g.dt * e_phi;\n    integ[N + e] = i_theta + g.dt * e_theta;\n    integ[2 * N + e] = i_va + g.dt * e_va;\n",
         "    integ[e] = i_phi;\n    integ[N + e] = i_theta;\n    integ[2 * N + e] = i_va;\n")],
    # ---- the device flight recorder (fwgym_record.h); they run the emulated forms, tests/test_recorder.py.
    # an episode end leaves the slabs where they are: the next episode overwrites the completed one
    "recorder_no_slab_flip": [
        ("fwgym_record.h", "    f = (f & ~(FWG_REC_F_OVERFLOW | FWG_REC_F_OPEN)) ^ FWG_REC_F_SLAB;", "    f = (f & ~(FWG_REC_F_OVERFLOW | FWG_REC_F_OPEN));")],
    # after an auto-reset the new episode's row 0 is not written (the other slab keeps an older episode's row 0)
    "recorder_row0_not_rewritten": [
        ("fwgym_record.h", "    } else if (reopen) {\n", "    } else if (reopen && false) {\n")],
    # the terminal row takes its state words from the arena under auto-reset too (the NEXT episode's reset state)
    "recorder_terminal_state_under_auto_reset": [
        ("fwgym_record.h", "    const bool state = !d || (!rc.auto_reset && (tc == FWG_TERM_STEPS || tc == FWG_TERM_SUCCESS));",
         "    const bool state = !d || (tc == FWG_TERM_STEPS || tc == FWG_TERM_SUCCESS);")],
    # store_derived off in turbulence: Va read where store_derived would keep it (a word the step does not write then)
    "recorder_turbulent_va_from_the_first_group": [
        ("fwgym_record.h", "return rec_arena(S, N, e, rc.derived + (i == 3 ? 6 : i));", "return rec_arena(S, N, e, rc.derived + i);")],
    # ---- the device training monitor (fwgym_monitor.h); they run the emulated forms, tests/test_monitor.py.
    # a done inside a segment emits the episode but leaves the running sums where they are
    "monitor_carry_not_cleared_at_a_done": [
        ("fwgym_monitor.h", "                    q = 0; len = 0;\n                }\n", "                }\n")],
    # the reward of the step that ends an episode goes to the next one
    "monitor_done_reward_to_the_next_episode": [
        ("fwgym_monitor.h", "                q += qk;\n", "                if (!d[k]) q += qk;\n"),
        ("fwgym_monitor.h", "                    q = 0; len = 0;\n                }\n", "                    q = qk; len = 0;\n                }\n")],
    # the lanes past the last env (they load env N - 1's values) emit its episodes once more
    "monitor_lanes_past_n_counted": [
        ("fwgym_monitor.h", "                if (d[k] && valid) {", "                if (d[k]) {")],
    # the bad flag of an episode stays set in the episode that follows it
    "monitor_bad_flag_survives_the_done": [
        ("fwgym_monitor.h", "                    q = 0; len = 0;\n                }\n", "                    q = 0; len &= FWG_MON_BAD;\n                }\n")],
    # ---- the goal env (fwgym_goal.h); they run the emulated forms, the kernel tests of tests/test_goal.py.
    # the substituted error of an angle without the wrap
    "goal_error_without_the_wrap": [
        ("fwgym_goal.h", "err[k] = target_error(c.target[k], tgt[i], val[i]);", "err[k] = c.target[k].wrap ? val[i] - tgt[i] : tgt[i] - val[i];")],
    # R one row too far: the future goal may come from the row behind the episode's last one, across a done
    "goal_future_row_across_a_done": [
        ("fwgym_goal.h", "            const long R = later != 0u ? t + __ffsll((long long)later) : after;",
         "            const long R = min(T, (later != 0u ? t + (long)__ffsll((long long)later) : after) + 1);")],
    # the action window of the delta factor not cut at the episode's first action
    "goal_window_not_cut_at_the_episode_start": [
        ("fwgym_goal.h", "                    const int m = (int)min(step + 1u, (unsigned)F.window);", "                    const int m = F.window;")],
    # ---- the hindsight replay buffer (fwgym_replay.h); they run the emulated forms, the kernel tests of tests/test_replay.py.
    # a future row that may reach one row past R (capped at the slot's last row): the goal may come from across a done
    "replay_future_row_past_the_episode": [
        ("fwgym_replay.h", "            src = (int)(s0 + 1 + (long)__umulhi(b.x, (unsigned)(R - s0)));",
         "            src = (int)min(T, s0 + 1 + (long)__umulhi(b.x, (unsigned)(R - s0 + 1)));")],
    # the slot drawn over the K allocated slots instead of the n_filled that hold a rollout
    "replay_slot_drawn_over_all_slots": [
        ("fwgym_replay.h", "        const long k = (long)__umulhi(a.x, A.n_filled);", "        const long k = (long)__umulhi(a.x, A.n_slots);")],
    # ---- the off-policy update (fwgym_offpolicy.h), arithmetic only and in bounds: plausible slips of a rewrite for speed; they run
    # the emulated forms of tests/test_offpolicy_contract.py.  With more tiles than workgroups every workgroup takes ntiles / gridDim.x
    # tiles and the remainder is dropped (equal to the even split up to 256 tiles): in the critics' kernel ...
    "ddpg_critic_grad_drops_remainder_tiles": [
        ("fwgym_offpolicy.h", "t1 = (long)(blockIdx.x + 1) * G.ntiles / gridDim.x;\n    DdpgAcc g[2];",
         "t1 = t0 + G.ntiles / gridDim.x;\n    DdpgAcc g[2];")],
    # ... and in the actor's
    "ddpg_actor_grad_drops_remainder_tiles": [
        ("fwgym_offpolicy.h", "t1 = (long)(blockIdx.x + 1) * G.ntiles / gridDim.x;\n    DdpgAcc g, none;",
         "t1 = t0 + G.ntiles / gridDim.x;\n    DdpgAcc g, none;")],
    # the two learning rates swapped
    "ddpg_apply_swaps_learning_rates": [
        ("fwgym_offpolicy.h", "    const double lr = seg ? h.lr_critic : h.lr_actor;", "    const double lr = seg ? h.lr_actor : h.lr_critic;")],
    # the two clip norms swapped
    "ddpg_apply_swaps_clip_norms": [
        ("fwgym_offpolicy.h", "    const float max_norm = (float)(seg ? h.max_norm_critic : h.max_norm_actor);",
         "    const float max_norm = (float)(seg ? h.max_norm_actor : h.max_norm_critic);")],
    # the fourth word of a goal row never read (every goal the env makes today has three)
    "ddpg_gather_drops_goal_word_3": [
        ("fwgym_offpolicy.h", "            else if (f < L.Ka) v = goal[row * FWG_DDPG_GOAL_STRIDE + f - L.D];",
         "            else if (f < L.Ka) v = f - L.D < 3 ? goal[row * FWG_DDPG_GOAL_STRIDE + f - L.D] : 0.f;")],
    # the actor's step counter in both segments' bias correction (and written back to the segment's own)
    "ddpg_apply_bias_correction_of_step_0": [
        ("fwgym_offpolicy.h", "    const int t = step[seg] + 1;", "    const int t = step[0] + 1;")],
    # the first layer's weight gradient without its columns 32 .. 63
    "ddpg_backward_skips_w1_columns_from_32": [
        ("fwgym_offpolicy.h", "        if (tn0 < K) ppo_mma_tile<true>(g.w1,", "        if (tn0 < K && tn0 < 32) ppo_mma_tile<true>(g.w1,")],
    # ---- the behaviour head (fwgym_behaviour.h); they run the emulated forms of tests/test_behaviour.py.  The per-env draw counter
    # read but not advanced: every act repeats the first one's noise
    "behaviour_draw_counter_not_advanced": [
        ("fwgym_behaviour.h", "        B.draws[e] = c + 1u;", "        B.draws[e] = c;")],
    # the goal columns gathered one word off (in bounds for the goal widths the tests use, G <= 3: word 3 of a row is the last read)
    "behaviour_goal_columns_one_word_off": [
        ("fwgym_behaviour.h", "    ddpg_gather(Xs, L, B.obs, goal, nullptr, r0, nrows, tid);", "    ddpg_gather(Xs, L, B.obs, goal + 1, nullptr, r0, nrows, tid);")],
}
_ORACLE_TESTS = ["-k", "not frozen_kernel_through", os.path.join(ROOT, "tests", "test_emu_coverage.py"),
                 os.path.join(ROOT, "tests", "test_emu_fuzz.py")]
_LEARNER_TESTS = ["-m", "not gpu", os.path.join(ROOT, "tests", "test_ppo_hip_contract.py")]
# (the regime in which prepared draws are completed, and the seed change: the 45-step regime never holds a complete draw)
_CURRICULUM_TESTS = ["-k", "sparse or another_seed", os.path.join(ROOT, "tests", "test_emu_curriculum.py")]
# the pytest arguments each mutant runs in `emu` mode
_HEAD_TESTS = ["-m", "not gpu", os.path.join(ROOT, "tests", "test_actor_contract.py")]
_CNN_LEARNER_TESTS = ["-m", "not gpu", os.path.join(ROOT, "tests", "test_ppo_hip_cnn.py")]
_EVAL_TESTS = [os.path.join(ROOT, "tests", "test_eval_device.py")]
_RECORDER_TESTS = [os.path.join(ROOT, "tests", "test_recorder.py")]
_MONITOR_TESTS = ["-k", "restatement or bad_reward or carries or sharded", os.path.join(ROOT, "tests", "test_monitor.py")]
_REPLAY_TESTS = ["-k", "restatement or seed_and_serial or backward_scan", os.path.join(ROOT, "tests", "test_replay.py")]
_GOAL_TESTS = ["-k", "matches_the_restatement or golden or own_goals or sharded", os.path.join(ROOT, "tests", "test_goal.py")]
_HEAD_CNN_TESTS = ["-m", "not gpu", os.path.join(ROOT, "tests", "test_actor_contract_cnn.py")]
_OFFPOLICY_TESTS = ["-m", "not gpu", os.path.join(ROOT, "tests", "test_offpolicy_contract.py")]
_BEHAVIOUR_TESTS = ["-m", "not gpu", os.path.join(ROOT, "tests", "test_behaviour.py")]
TESTS = {name: (_BEHAVIOUR_TESTS if name.startswith("behaviour_") else _OFFPOLICY_TESTS if name.startswith("ddpg_") else _REPLAY_TESTS if name.startswith("replay_") else _GOAL_TESTS if name.startswith("goal_") else _MONITOR_TESTS if name.startswith("monitor_") else _RECORDER_TESTS if name.startswith("recorder_") else _EVAL_TESTS if name.startswith("eval_") else _HEAD_CNN_TESTS if name.startswith("head_cnn_") else _CNN_LEARNER_TESTS if name.startswith("ppo_cnn_") else _LEARNER_TESTS if name.startswith(("ppo_", "actor_pack_")) else _HEAD_TESTS if name.startswith("head_") else
                _CURRICULUM_TESTS if name.endswith("_generation") else _ORACLE_TESTS) for name in MUTANTS}
# (a level change moves no range the per-env sets are drawn from: a kept set equals a new draw, and only the seed change shows this one)
TESTS["model_draw_ignores_generation"] = ["-k", "another_seed", os.path.join(ROOT, "tests", "test_emu_curriculum.py")]


def mutated_tree(name):
    d = tempfile.mkdtemp(prefix="fwg_mut_{}_".format(name))
    dst = os.path.join(d, "fixed-wing-gym_amd", "csrc")
    shutil.copytree(CSRC, dst)
    shutil.copytree(os.path.join(ROOT, "include"), os.path.join(d, "include"))
    for fn, old, new in MUTANTS[name]:
        p = os.path.join(dst, fn)
        s = open(p).read()
        assert s.count(old) == 1, "mutation site of {} not found exactly once in {}: the source moved, update tools/mutation_check.py".format(name, fn)
        open(p, "w").write(s.replace(old, new))
    return d, dst


def _hip_mutant(job):
    name, layout, outdir = job
    sys.path[:0] = [ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests")]
    import copy
    from gym_fixed_wing import jit, presets
    d, dst = mutated_tree(name)
    cache = tempfile.mkdtemp(prefix="fwg_mutcache_")
    jit.CSRC, jit.CACHE = dst, cache
    cfg, ckw, skw, _, _ = presets.workload("c3")
    # (layout "curriculum" / "curriculum_model16": the row-log configurations of the curriculum runs of
    # tests/test_gpu_oracle_coverage.py -- c3_sparse_log with its 181-step episodes, c3_model16_lean_log with per-env aircraft)
    if layout == "curriculum_model16":
        cfg = presets.preset("cnn_model16")
    ckw = dict(copy.deepcopy(ckw), steps_max=181 if layout == "curriculum" else 45,
               simulator={"states": {6: {"constraint_min": -60, "constraint_max": 60}}})
    lib = jit.prebuild(cfg, ckw, skw, derived_views=False, obs_log_rows=0 if layout == "dense" else presets.OBS_LOG_ROWS)
    assert lib is not None, (name, layout)
    out = os.path.join(outdir, "libfwgym_mut_{}_{}.so".format(name, layout))
    shutil.move(lib, out)
    shutil.rmtree(d), shutil.rmtree(cache)
    return out


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "emu"
    if mode == "hip":
        # the fail-prone steady-state configuration of tests/test_gpu_oracle_coverage.py, frozen (jit.py's build recipe) from the
        # mutated sources, row log and dense: libfwgym_mut_<name>_<layout>.so under OUTDIR
        outdir = os.path.abspath(sys.argv[2])
        os.makedirs(outdir, exist_ok=True)
        sys.path[:0] = [ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests")]
        import copy
        from concurrent.futures import ProcessPoolExecutor
        jobs = [(name, layout, outdir) for name in ("airdata", "install_on_failed_last_step") for layout in ("row_log", "dense")]
        # FWGYM_MUTANT_LIB_CURRICULUM / FWGYM_MUTANT_LIB_CURRICULUM_MODEL16 point the curriculum runs at these.  The first must be
        # caught there (c3_sparse_log).  The second is EXPECTED TO SURVIVE c3_model16_lean_log: a level change moves no range the
        # per-env sets are drawn from, so a set kept across it equals a new draw; only a seed change shows that mutant
        # (tests/test_emu_curriculum.py, the `another_seed` tests).  It is built so that a GPU session can confirm this
        jobs += [("draw_ready_ignores_generation", "curriculum", outdir), ("model_draw_ignores_generation", "curriculum_model16", outdir)]
        with ProcessPoolExecutor(max_workers=4) as pool:
            for out in pool.map(_hip_mutant, jobs):
                print("built", out)
        return 0
    sys.path[:0] = [ROOT, os.path.join(ROOT, "fixed-wing-gym_amd"), os.path.join(ROOT, "tests")]
    caught = {}
    for name in (sys.argv[2:] or MUTANTS):
        d, dst = mutated_tree(name)
        env = dict(os.environ, FWGYM_MUTANT_SRC=dst, FWGYM_MUTANT_TAG="_mut_" + name)
        r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider"] + TESTS[name],
                           env=env, capture_output=True, text=True)
        caught[name] = r.returncode != 0
        tail = [l for l in r.stdout.splitlines() if "Mismatch" in l or "FAILED" in l or "passed" in l or "failed" in l][-6:]
        print("mutant {:32s} {}".format(name, "CAUGHT" if caught[name] else "SURVIVED"))
        for l in tail:
            print("    " + l[:220])
        shutil.rmtree(d)
        for f in os.listdir(os.path.join(ROOT, "tests", "emu")):
            if "_mut_" in f:
                os.remove(os.path.join(ROOT, "tests", "emu", f))
    return 0 if all(caught.values()) else 1


if __name__ == "__main__":
    sys.exit(main())
