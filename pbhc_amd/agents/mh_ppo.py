"""MHPPO — drop-in for the reference's KungfuBot PPO (multi-head / vector-reward critic).

Same class surface as the reference (reference: humanoidverse/agents/mh_ppo/mh_ppo.py:26-775 on the
BaseAlgo API agents/base_algo/base_algo.py:15-47): `__init__(env, config, log_dir=None, device)`,
`setup()`, `load(path)`, `save(path, infos)`, `learn()`, `evaluate_policy()`, `inference_model`;
checkpoint dict and state_dict key names are the reference's, so trained policies still export and
deploy through the reference's tooling.  Select with
`algo._target_: pbhc_amd.agents.mh_ppo.MHPPO`.

MI355X-first differences (same maths, pinned by tests/golden/ppo_v1.npz):
  * no host synchronisation inside an iteration: the adaptive-KL learning rate, the loss meters and
    the episode statistics live on the device (`torch.where`, capturable Adam with tensor lr);
  * GAE / head-summed advantage / normalisation run in `pbhc_gae` (HIP) on the `[T,N,R]` slab;
  * the minibatch gather moves only the keys the update reads;
  * envs shard over ranks (one process per GPU): ONE flat-bucket RCCL all-reduce of the actor+critic
    gradients per optimiser step, plus two tiny all-reduces (advantage moments, KL mean) so that
    every rank takes the same normalisation and learning-rate branch as one big batch would.

What it shares with ppo_mimic.PPO is agents/base.py; the rollout is agents/rollout.py.
"""
from __future__ import annotations

import ctypes as C

import torch

from .. import _lib
from .. import dist as pdist
from . import fused_mlp, rollout
from .base import FlatAdamView, OnDeviceAgent, _load_checkpoint, switch, switch_on
from .modules import BaseModule, PPOActor, PPOCritic


class MHPPO(OnDeviceAgent):
    def _init_config(self):
        super()._init_config()
        c = self.config
        self.actor_learning_rate = c.actor_learning_rate
        self.critic_learning_rate = c.critic_learning_rate
        self.cfg_l2c2 = c.l2c2 if "l2c2" in c else None
        sym = c.get("symmetry", None)
        if sym is not None and sym.get("enable", False):
            raise NotImplementedError("algo.config.symmetry.enable with MHPPO: the mirror-symmetry term belongs to the general-tracking agent "
                                      "(ppo_mimic.PPO) — a v1 library is one clip and has no mirrored variant to tie the policy to")

    # ------------------------------------------------------------------------------------
    def _setup_models_and_optimizer(self):
        c = self.config
        if "phase_embed" in c and c.phase_embed.type != "Original":
            # the reference's branch (mh_ppo.py:127-142) constructs `PhaseAwareActorV2` / `PhaseAwareCriticV2`, which no file of the reference
            # defines or imports: it raises NameError there, so there is no behaviour to reproduce
            raise NotImplementedError("phase_embed.type != 'Original': the reference's PhaseAwareActorV2 / PhaseAwareCriticV2 do not exist (mh_ppo.py:127-142)")
        c.module_dict.critic["output_dim"][-1] = self.num_rew_fn
        self.actor = PPOActor(obs_dim_dict=self.algo_obs_dim_dict, module_config_dict=c.module_dict.actor, num_actions=self.num_act,
                              init_noise_std=c.init_noise_std).to(self.device)
        self.critic = PPOCritic(obs_dim_dict=self.algo_obs_dim_dict, module_config_dict=c.module_dict.critic).to(self.device)
        if self._dp:      # replicas start from rank 0's weights
            for p in list(self.actor.parameters()) + list(self.critic.parameters()):
                pdist.broadcast(p.data, src=0)
        self._flatten_parameters()

    def _flatten_parameters(self):
        """All actor+critic parameters (and their grads / Adam moments) live in ONE flat fp32 buffer each:
        one RCCL all-reduce over the gradient bucket, one clip+Adam launch per network."""
        dev = self.device
        pa, pc = list(self.actor.parameters()), list(self.critic.parameters())
        self._params = pa + pc
        self._n_actor = sum(p.numel() for p in pa)
        self._n_critic = sum(p.numel() for p in pc)
        n = self._n_actor + self._n_critic
        self._pflat = torch.zeros(n, device=dev)
        self._gflat = torch.zeros(n + 1, device=dev)         # + one slot behind the critic's segment: the minibatch KL rides in its all-reduce
        self._mflat = torch.zeros(n, device=dev)
        self._vflat = torch.zeros(n, device=dev)
        o = 0
        self._slices = []
        for p in self._params:
            k = p.numel()
            self._pflat[o:o + k].copy_(p.data.reshape(-1))
            p.data = self._pflat[o:o + k].view_as(p)
            p.grad = self._gflat[o:o + k].view_as(p)
            self._slices.append((o, k))
            o += k
        std_idx = [i for i, (nme, _) in enumerate(self.actor.named_parameters()) if nme == "std"][0]
        self._std_slice = self._slices[std_idx]
        self._lr = torch.tensor([float(self.actor_learning_rate), float(self.critic_learning_rate)], device=dev)
        self._lr_a, self._lr_c = self._lr[0:1], self._lr[1:2]
        self._adam_step = torch.zeros(2, device=dev)          # [actor, critic] step counts (float, like torch's `step` tensors)
        self._adam_scratch = torch.zeros(2, 512, dtype=torch.float64, device=dev)
        self._grad_norms = torch.zeros(2, device=dev)
        self._finish_plan = None                              # set by _update_ppo for the _adam2 call that follows it (see there)
        self._loss_scalars = torch.zeros(4, device=dev)
        self.betas, self.adam_eps = (0.9, 0.999), 1e-8
        # kept for checkpoint (de)serialisation in torch.optim.Adam's format
        entries = [(o, k, p.shape, True) for (o, k), p in zip(self._slices, self._params)]
        view = lambda i, ent: FlatAdamView(self, ent, self._mflat, self._vflat, self._adam_step[i:i + 1], self._lr[i:i + 1], keep_unstepped=True)
        self.actor_optimizer, self.critic_optimizer = view(0, entries[:len(pa)]), view(1, entries[len(pa):])
        # every update zeroes `_gflat` before its backward: the MLP stacks may store their gradients into it directly
        self._direct_stacks = []
        for m in list(self.actor.modules()) + list(self.critic.modules()):
            if isinstance(m, BaseModule):
                fused_mlp.grad_direct(m.module)
                self._direct_stacks.append(m.module)

    def _zero_grads(self):
        """zero the flat gradient buffer and tell the declared stacks (their next backward may store instead of accumulate)"""
        # INVARIANT behind the shortcut: between the Adam pass of one optimiser step (pbhc_adam_clip2(zero_grad=1) leaves the buffer zeroed)
        # and this call nothing runs a backward through a module whose .grad views the flat buffer.  _update_ppo is the only writer on the
        # training path; load() and the eager update clear the flag; PBHC_CHECK_GRAD_CLEAN=1 verifies it (one reduction + a sync per step).
        if getattr(self, "_gflat_clean", False) and switch_on("PBHC_CHECK_GRAD_CLEAN"):
            assert float(self._gflat[: self._n_actor + self._n_critic].abs().sum()) == 0.0, "a gradient was written outside _update_ppo"
        if not getattr(self, "_gflat_clean", False):      # (clean: the last Adam pass left it zeroed and nothing has written it since)
            self._gflat.zero_()
        self._gflat_clean = False
        for q in self._direct_stacks:
            fused_mlp.grads_zeroed(q)

    def _setup_storage(self):
        self._need_next = bool(self.cfg_l2c2 is not None and self.cfg_l2c2.enable)
        if self._need_next:                      # the L2C2 terms run each network twice per graph: plain autograd accumulation
            self.actor.actor_module._fused = False
            self.critic.critic_module._fused = False
        obs = self.algo_obs_dim_dict
        self._register_storage(obs, {"next_" + k: d for k, d in obs.items()} if self._need_next else {})

    def _eval_mode(self):
        self.actor.eval(); self.critic.eval()

    def _train_mode(self):
        self.actor.train(); self.critic.train()

    # ---- checkpoints: the reference's dict (mh_ppo.py:176-204) -----------------------------
    def load(self, ckpt_path):
        if ckpt_path is None:
            return None
        d = _load_checkpoint(ckpt_path, self.device)
        self._gflat_clean = False            # (whatever touched the gradients meanwhile: the next update zeroes the flat buffer itself)
        self.actor.load_state_dict(d["actor_model_state_dict"])
        self.critic.load_state_dict(d["critic_model_state_dict"])
        if self.load_optimizer:
            self.actor_optimizer.load_state_dict(d["actor_optimizer_state_dict"])
            self.critic_optimizer.load_state_dict(d["critic_optimizer_state_dict"])
            self.set_learning_rate(float(d["actor_optimizer_state_dict"]["param_groups"][0]["lr"]),
                                   float(d["critic_optimizer_state_dict"]["param_groups"][0]["lr"]))
        self.current_learning_iteration = d["iter"]
        self._restore_training_state(d)
        return d["infos"]

    def save(self, path, infos=None):
        torch.save(self._with_training_state({
            "actor_model_state_dict": self.actor.state_dict(),
            "critic_model_state_dict": self.critic.state_dict(),
            "actor_optimizer_state_dict": self.actor_optimizer.state_dict(),
            "critic_optimizer_state_dict": self.critic_optimizer.state_dict(),
            "iter": self.current_learning_iteration,
            "infos": infos,
        }), path)

    def set_learning_rate(self, actor_learning_rate, critic_learning_rate):
        self.actor_learning_rate, self.critic_learning_rate = actor_learning_rate, critic_learning_rate
        self._lr[0] = float(actor_learning_rate)
        self._lr[1] = float(critic_learning_rate)

    # ---- learn loop (mh_ppo.py:206-250) ----------------------------------------------------
    def learn(self, num_iterations=None):
        self._learn_loop(num_iterations, self._rollout_step, self._training_step)

    def _actor_act_step(self, obs_dict):
        return self.actor.act(obs_dict["actor_obs"])

    def _critic_eval_step(self, obs_dict):
        return self.critic.evaluate(obs_dict["critic_obs"])

    def _critic_values(self, obs_dict):          # the bootstrap values of GAE when the rollout did not leave them
        return self._critic_eval_step(obs_dict)

    def _prefetch_permutation(self, n):
        """The update's minibatch permutation (data_utils.py:139, `torch.randperm(batch_size)`) does not depend on the rollout's data: its
        ten sort launches (~125 us) are queued on a stream of their own before the rollout starts and run beside it.  Same generator, same
        draw per iteration — nothing else draws from torch's device generator in between (policy sampling and env resets are Philox streams
        keyed by their own counters)."""
        if not switch_on("PBHC_PERM_PREFETCH"):
            return
        if self.__dict__.get("_perm_stream") is None:
            self._perm_stream = torch.cuda.Stream(device=self.device)
            self._perm_buf = torch.empty(n, dtype=torch.int64, device=self.device)
        if self._perm_buf.numel() != n:
            self._perm_buf = torch.empty(n, dtype=torch.int64, device=self.device)
        ps = self._perm_stream
        ps.wait_stream(torch.cuda.current_stream())           # (the previous update's gather has read the buffer)
        with torch.cuda.stream(ps):
            torch.randperm(n, device=self.device, out=self._perm_buf)
        self._perm_event = ps.record_event()

    def _take_permutation(self, n):
        ev = self.__dict__.get("_perm_event")
        if ev is None or self._perm_buf.numel() != n:
            return None
        self._perm_event = None
        torch.cuda.current_stream().wait_event(ev)
        return self._perm_buf

    def _rollout_step(self, obs_dict):
        """mh_ppo.py:270-342 through agents/rollout.py: the actor stack (PBHC_STACK_NETS names the networks that run from packed weights) with
        the sampling in its last epilogue; the critic over all slabs after the loop, or (PBHC_CRITIC_BATCHED=0) the critic of slab t on the
        branch stream next to the actor, one hipGraph launch per step.  ONE hipGraph for the loop in the default form, never with L2C2."""
        st, env = self.storage, self.env
        self._prefetch_permutation(self.num_steps_per_env * env.num_envs)
        batched = rollout.critic_batched(env)
        std, a_mod, c_mod = self.actor.std, self.actor.actor_module, self.critic.critic_module
        nets = [n_ for n_ in switch("PBHC_STACK_NETS").split(",") if n_ and not (batched and n_ == "critic")]
        P = lambda x: x.data_ptr()

        def forward(t):
            if not d.fuse_sample:
                return a_mod(st.actor_obs[t]), None
            if not fused_mlp.forward_sample(a_mod.module, st.actor_obs[t], std, self._sample_seed, self._ctr0.data_ptr(), t, st.actions[t], st.action_mean[t],
                                            st.action_sigma[t], st.actions_log_prob[t], riders=d.rider):
                raise _lib.PbhcError("pbhc_mlp_fwd_sample does not apply to this policy (PBHC_FUSED_SAMPLE=0)")
            return st.action_mean[t], None

        def keep_next(t, nxt):
            for k in d.keys:
                getattr(st, "next_" + k)[t].copy_(nxt[k])

        d = rollout.RolloutSpec(
            keys=list(obs_dict.keys()), batched=batched, forward=forward, early_fwd_graphs=True, sigma=std, sample_stack=a_mod.module,
            stacks=[m.module for n_, m in (("actor", a_mod), ("critic", c_mod)) if n_ in nets and m._fused],
            critic_step=None if batched else lambda t: c_mod(st.critic_obs[t]),
            graph_allowed=lambda: batched and d.fuse_sample and not self._need_next,
            sample_ptrs=lambda t: (P(st.actions[t]), P(st.action_mean[t]), P(st.action_sigma[t]), P(st.actions_log_prob[t]), None),
            critic=c_mod, critic_rows=lambda: st.with_tail("critic_obs").flatten(0, 1), after_step=keep_next if self._need_next else None)
        return rollout.collect(self, d, obs_dict)

    # ---- update (mh_ppo.py:397-533) --------------------------------------------------------
    UPDATE_KEYS = ["actor_obs", "critic_obs", "actions", "values", "advantages", "returns", "actions_log_prob", "action_mean", "action_sigma"]
    METERS = ["Value", "Surrogate", "Entropy", "L2C2_Value", "L2C2_Policy"]

    def _training_step(self, indices=None):
        meters, loss = self._begin_meters(self.METERS)
        keys = self.UPDATE_KEYS + (["next_actor_obs", "next_critic_obs"] if self._need_next else [])
        if indices is None:
            indices = self._take_permutation(self.storage.num_envs * self.storage.num_transitions_per_env)      # (None: drawn by the generator now)
        for batch in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, keys=keys, indices=indices):
            self._update_ppo(batch, loss)
        self.actor_learning_rate = self._lr_a        # tensors; read back lazily by the logger
        self.critic_learning_rate = self._lr_c
        return self._end_meters(self.METERS, meters, loss)

    def _allreduce_grads(self):
        """ONE RCCL all-reduce of the flat actor+critic gradient buffer (≈5 MB fp32), then average."""
        pdist.allreduce_mean_(self._gflat)

    def _adam2(self, zero_grad):
        """both networks' clip_grad_norm_ + Adam in one launch pair (two segments of the flat buffers, each clipped by its own norm);
        zero_grad: the pass leaves the gradient buffer zeroed — the next step's zero_grad().
        Where the backward's finishing launch has just left the gradient's sums of squares (`_finish_plan`, a fused_mlp.StepSqnorm.Plan set
        by _update_ppo for this one call): the optimiser pass alone on those partials — no norm launch, and the step counters were
        advanced by that launch.  (The plan comes by the attribute, consumed here, and not as a parameter: `_adam2(zero_grad)` is the one
        hook of the optimiser pass, and what wraps it — tests/test_gpu_update_tail.py keeps the gradients through it — has that signature.)"""
        plan, self._finish_plan = self._finish_plan, None
        lib, P = _lib.lib(), lambda t: t.data_ptr()
        if plan is not None:
            _lib.check(lib.pbhc_adam_clip2_parts(P(self._pflat), P(self._gflat), P(self._mflat), P(self._vflat), self._n_actor, self._n_critic, P(self._lr),
                                                 P(self._adam_step), float(self.max_grad_norm), self.betas[0], self.betas[1], self.adam_eps, 0.0, zero_grad,
                                                 plan.part_ptr[0], plan.nparts[0], plan.part_ptr[1], plan.nparts[1], P(self._grad_norms),
                                                 _lib.current_stream()), "pbhc_adam_clip2_parts")
            return
        _lib.check(lib.pbhc_adam_clip2(P(self._pflat), P(self._gflat), P(self._mflat), P(self._vflat), self._n_actor, self._n_critic, P(self._lr),
                                       P(self._adam_step), float(self.max_grad_norm), self.betas[0], self.betas[1], self.adam_eps, 0.0, zero_grad,
                                       P(self._adam_scratch), P(self._grad_norms), _lib.current_stream()), "pbhc_adam_clip2")

    def _update_ppo(self, b, loss):
        if self._need_next:
            return self._update_ppo_eager(b, loss)
        lib = _lib.lib()
        # One stream for both networks: with the critic on a stream of its own the update measured 37.0 ms against 34.5 ms (MI355X, 4096 envs) —
        # the wide GEMMs are tuned to own the chip and lose more than the narrow ones gain.
        # Both stacks as one autograd node where their 128-wide tails can share launches (fused_mlp.forward_pair; PBHC_PAIR_TAILS=0: never),
        # else each on its own; `_update_form` says which.  The paired form also pairs the wide layers' forwards where both stacks' run on
        # 64 x 128 tiles (PBHC_PAIR_WIDE=0: never); `_update_pairs` lists the kinds of those pairs this step issued.
        am, cm = self.actor.actor_module, self.critic.critic_module
        pair = None
        self._update_pairs = []
        launches0 = fused_mlp.LAUNCHES[0]
        if switch_on("PBHC_PAIR_TAILS") and am._fused and cm._fused:
            pair = fused_mlp.forward_pair(am.module, b["actor_obs"], cm.module, b["critic_obs"], wide=switch_on("PBHC_PAIR_WIDE"), formed=self._update_pairs)
        self._update_form = "per-stack" if pair is None else "paired"
        mu, value = pair if pair is not None else (am(b["actor_obs"]), cm(b["critic_obs"]))
        B = mu.shape[0]
        if B != self._mb:
            raise _lib.PbhcError("minibatch size changed")
        self._zero_grads()
        so, sn = self._std_slice
        adapt = int(self.desired_kl is not None and self.schedule == "adaptive")
        on_device_lr = adapt if not self._dp else 0
        st = _lib.current_stream()
        # The loss's first stage here; its one-workgroup second stage (d(loss)/d(std), the loss scalars, the learning-rate rule) rides in the
        # backward's finishing launch: nothing reads its results before the all-reduce / the optimiser pass.
        npart = C.c_int(0)
        _lib.check(lib.pbhc_ppo_loss_partials(mu.data_ptr(), self.actor.std.data_ptr(), value.data_ptr(), b["actions"].data_ptr(), b["actions_log_prob"].data_ptr(),
                                              b["action_mean"].data_ptr(), b["action_sigma"].data_ptr(), b["advantages"].data_ptr(), b["returns"].data_ptr(),
                                              b["values"].data_ptr(), B, self.num_act, self.num_rew_fn, float(self.clip_param), float(self.value_loss_coef),
                                              int(self.use_clipped_value_loss), 0, self._grad_mu.data_ptr(), self._grad_value.data_ptr(),
                                              self._loss_scratch.data_ptr(), C.byref(npart), st), "pbhc_ppo_loss_partials")
        red = _lib.PbhcPpoReduce()
        red.scratch, red.std, red.grad_std = self._loss_scratch.data_ptr(), self.actor.std.data_ptr(), self._gflat[so:so + sn].data_ptr()
        red.scalars, red.scalars_acc, red.lr = self._loss_scalars.data_ptr(), loss["_acc"].data_ptr() if "_acc" in loss else None, self._lr.data_ptr()
        red.num_partials, red.B, red.A, red.adapt_lr = npart.value, B, self.num_act, on_device_lr
        red.entropy_coef, red.desired_kl = float(self.entropy_coef), float(self.desired_kl or 0.0)
        # The gradient norm: every gradient element is produced or passed by the backward's finishing launch, which squares what it stores
        # (PBHC_STEP_FINISH=0: a norm pass of its own over the flat buffer, as _adam2 runs it).  Not data-parallel: the all-reduce changes the
        # gradients after the finish, so the norm has to follow it.  `_step_finish` says which form ran; `_update_launches` is the step's
        # launch count by bookkeeping (fused_mlp.LAUNCHES at its call sites + this method's own: loss, (norm,) Adam, the data-parallel
        # copy / all-reduce / rule) — not read from the stream.
        sqnorm = None
        if switch_on("PBHC_STEP_FINISH") and not self._dp and am._fused and cm._fused and all(getattr(q, "_grad_direct", False) for q in self._direct_stacks):
            if self.__dict__.get("_sqnorm") is None or self._sqnorm.gflat is not self._gflat:
                self._sqnorm = fused_mlp.StepSqnorm(self._gflat, self._n_actor, self._n_critic, self._adam_step)
            sqnorm = self._sqnorm
        plan = self._backward_both(mu, value, red, sqnorm)
        self._step_finish = "squares" if plan is not None else "norm-pass"
        na, nc = self._n_actor, self._n_critic
        if self._dp:
            # ONE all-reduce per optimiser step (north_star: "a single RCCL all-reduce of policy gradients per PPO update"): actor + critic
            # segments and, in the slot behind them, the minibatch KL mean (the adaptive learning-rate rule, mh_ppo.py:455-466, needs the
            # mean over ALL ranks' samples) — averaged by the collective itself (ReduceOp.AVG), 5.2 MB, latency-bound on xGMI.
            self._gflat[na + nc:na + nc + 1].copy_(self._loss_scalars[3:4])      # (behind the backward: its finishing launch leaves the KL mean)
            pdist.allreduce_mean_(self._gflat[:na + nc + 1])
            if adapt:                                    # the rule on the all-rank KL mean: one launch (pdist.kl_lr_rule_ is its host-tensor form)
                _lib.check(lib.pbhc_kl_lr_rule(self._lr.data_ptr(), 2, self._gflat[na + nc:].data_ptr(), float(self.desired_kl), st), "pbhc_kl_lr_rule")
        self._finish_plan = plan                          # (None: _adam2 runs its own norm pass)
        self._adam2(zero_grad=1)
        self._update_launches = fused_mlp.LAUNCHES[0] - launches0 + (3 if plan is None else 2) + ((2 + adapt) if self._dp else 0)   # + loss, (norm,) Adam
        self._gflat_clean = True
        if "_acc" not in loss:                            # ("_acc": summed by the loss's second stage)
            loss["Value"] += self._loss_scalars[1]; loss["Surrogate"] += self._loss_scalars[0]; loss["Entropy"] += self._loss_scalars[2]
        return loss

    def _backward_both(self, mu, value, reduce, sqnorm=None):
        """both networks' backward on this stream, their finishing column-sum launches merged into one (fused_mlp.finish_deferred) that also
        carries the loss's second stage (`reduce`, a PbhcPpoReduce) and, with `sqnorm` (a fused_mlp.StepSqnorm), leaves the gradient's sums of
        squares -> the StepSqnorm.Plan that ran, or None"""
        fused_mlp.begin_deferred_finish()
        plan = None
        try:
            torch.autograd.backward([mu, value], [self._grad_mu, self._grad_value])
        finally:
            plan = fused_mlp.finish_deferred(reduce, sqnorm)
        return plan

    def _update_ppo_eager(self, b, loss):
        """Eager PyTorch form of the update (used only for the optional L2C2 regulariser, mh_ppo.py:488-507)."""
        self.actor.update_distribution(b["actor_obs"])
        logp = self.actor.get_actions_log_prob(b["actions"])
        value = self.critic.evaluate(b["critic_obs"])
        mu, sigma, entropy = self.actor.action_mean, self.actor.action_std, self.actor.entropy
        if self.desired_kl is not None and self.schedule == "adaptive":
            with torch.no_grad():
                old_s, old_m = b["action_sigma"], b["action_mean"]
                kl = torch.sum(torch.log(sigma / old_s + 1.0e-5) + (old_s.square() + (old_m - mu).square()) / (2.0 * sigma.square()) - 0.5, axis=-1)
                kl_mean = kl.mean()
                if self._dp:
                    pdist.all_reduce(kl_mean)
                    kl_mean = kl_mean / self.world_size
                up = kl_mean > self.desired_kl * 2.0
                down = (kl_mean < self.desired_kl / 2.0) & (kl_mean > 0.0)
                self._lr.copy_(torch.where(up, torch.clamp(self._lr / 1.5, min=1e-5), torch.where(down, torch.clamp(self._lr * 1.5, max=1e-2), self._lr)))
        adv = b["advantages"].squeeze(-1)
        ratio = torch.exp(logp - b["actions_log_prob"].squeeze(-1))
        surrogate = torch.max(-adv * ratio, -adv * torch.clamp(ratio, 1.0 - self.clip_param, 1.0 + self.clip_param)).mean()
        if self.use_clipped_value_loss:
            vclip = b["values"] + (value - b["values"]).clamp(-self.clip_param, self.clip_param)
            value_loss = torch.max((value - b["returns"]).pow(2), (vclip - b["returns"]).pow(2)).sum(dim=-1).mean()
        else:
            value_loss = (b["returns"] - value).pow(2).sum(dim=-1).mean()
        entropy_loss = entropy.mean()
        l2c2_v = torch.zeros((), device=self.device)
        l2c2_p = torch.zeros((), device=self.device)
        if self._need_next:
            u = torch.rand(*b["actor_obs"].shape[:-1], 1, device=self.device) * 2 - 1
            u_mu = self.actor.act_inference(b["actor_obs"] + u * (b["next_actor_obs"] - b["actor_obs"]))
            u_val = self.critic.evaluate(b["critic_obs"] + u * (b["next_critic_obs"] - b["critic_obs"]))
            l2c2_v = self.cfg_l2c2.lambda_value * (value - u_val).pow(2).mean()
            l2c2_p = self.cfg_l2c2.lambda_policy * (b["actions"] - u_mu).pow(2).mean()
        actor_loss = surrogate - self.entropy_coef * entropy_loss + l2c2_p
        critic_loss = self.value_loss_coef * value_loss + l2c2_v
        self._zero_grads()
        actor_loss.backward()
        critic_loss.backward()
        if self._dp:
            self._allreduce_grads()
        self._adam2(zero_grad=0)
        with torch.no_grad():
            loss["Value"] += value_loss.detach(); loss["Surrogate"] += surrogate.detach(); loss["Entropy"] += entropy_loss.detach()
            loss["L2C2_Value"] += l2c2_v.detach(); loss["L2C2_Policy"] += l2c2_p.detach()
        return loss

    # ---- evaluation / export surface --------------------------------------------------------
    @property
    def inference_model(self):
        return {"actor": self.actor, "critic": self.critic}

    @torch.no_grad()
    def evaluate_policy_steps(self, Nsteps):
        self._eval_mode()
        self.env.set_is_evaluating()
        obs = self.env.reset_all()
        for _ in range(Nsteps):
            obs, _, _, _ = self.env.step({"actions": self.actor.act_inference(obs["actor_obs"])})
        return obs

    @torch.no_grad()
    def evaluate_library(self, **kw):
        """Score every unique clip of the motion library once under the current policy (env.library_sweep; **kw: its max_steps, sync_every,
        before_wave).  Leaves and returns `self.library_metrics`."""
        self._eval_mode()
        self.library_metrics = self.env.library_sweep(lambda obs: self.actor.act_inference(obs["actor_obs"]), **kw)
        return self.library_metrics

    def evaluate_policy(self):
        if getattr(self.env, "save_motion", False):
            return self._evaluate_and_record()
        return self.evaluate_policy_steps(int(self.env.max_episode_length))

    EVAL_GRAPH_STEPS = 24

    @torch.no_grad()
    def _evaluate_and_record(self):
        """env.config.save_motion on (eval_agent.py with +opt=record): the reference's evaluation loop is `while True`, and a person stops it
        once the env has dumped its recording; here the loop ends at the dump, i.e. when the recorder — which has been counting control steps
        since the env was built, as the reference's lists do — has seen save_total_steps + 3 of them.  The steps run as replays of ONE captured
        graph of up to EVAL_GRAPH_STEPS x (actor forward, fused env step, recorder frame) when the env allows it (`rollout_graph_safe`;
        PBHC_ROLLOUT_GRAPH=0 or a failed capture: the eager loop); the remainder, and the first step (online GEMM selection must not run inside
        a capture), run eagerly.  Leaves `self.eval_metrics`: the recording scored on the device (metrics.eval_batch_traj_device against the
        clip of env 0, as sample_eps.py) + `first_termination_ratio` (ratio_eps.py) of the recorded `terminate`."""
        from ..eval import metrics

        env = self.env
        self._eval_mode()
        env.set_is_evaluating()
        env.reset_all()
        one = lambda: env.step({"actions": self.actor.act_inference(env.obs_buf_dict["actor_obs"])})[0]
        total = env.layout.record["total_steps"] + 3
        if not env.motion_recorded:
            one()
        chunk = min(self.EVAL_GRAPH_STEPS, total - env.recorded_steps)
        self._eval_used_graph = False
        if chunk >= 2 and switch_on("PBHC_ROLLOUT_GRAPH") and env.rollout_graph_safe(chunk):
            # (one stream, no finalize stream: the env's own events are not part of this graph)
            with env.graph_steps(renew_events=False):
                got = rollout.capture_graphs(self, [lambda: [one() for _ in range(chunk)]], what="evaluation")
            while got is not None and total - env.recorded_steps >= chunk and env.rollout_graph_safe(chunk):
                got[0][0].replay()
                env.after_graph_steps(chunk)
                self._eval_used_graph = True
        while not env.motion_recorded:
            one()
        rec = env.recorded_motion_device()
        self.eval_metrics = metrics.eval_batch_traj_device(env.skeleton, rec, env.clip_of_env(0))
        self.eval_metrics["first_termination_ratio"] = metrics.first_termination_ratio(rec["terminate"].cpu().numpy())
        return env.obs_buf_dict

    # ---- logging ------------------------------------------------------------------------------
    def _log_scalars(self, w, it):
        w.add_scalar("Loss/actor_learning_rate", float(self._lr_a), it)
        w.add_scalar("Loss/critic_learning_rate", float(self._lr_c), it)
        w.add_scalar("Policy/mean_noise_std", float(self.actor.std.detach().mean()), it)

    def _log_line(self, loss_dict):
        return f"value {float(loss_dict['Value']):.4f}  surr {float(loss_dict['Surrogate']):.4f}  lr {float(self._lr_a):.2e}"
