"""PPO (ppo_mimic) — drop-in for the reference's KungfuBot2 general-tracking agent.

Same class surface as the reference (reference: humanoidverse/agents/ppo/ppo_mimic.py:34-975 on the BaseAlgo API):
`__init__(env, config, log_dir=None, device)`, `setup()`, `load(path)`, `save(path, infos)`, `learn()`, `inference_model`;
the checkpoint dict (`model_state_dict`, `optimizer_state_dict` in torch.optim.AdamW's format, `iter`, `infos`) and every
state_dict key are the reference's.  Select with `algo._target_: pbhc_amd.agents.ppo_mimic.PPO`.

Both branches of the reference are implemented: the teacher (RL) path — PPO on the privileged latent with the `priv_reg` term
and, every `dagger_update_freq` iterations, the DAgger regression of the history encoder (ppo_mimic.py:270-300,596-709) — and the
student distillation path (`teacher_model_path` set, `dagger_only: True`; ppo_mimic.py:121-191,313-357,533-549,711-724): the frozen
teacher actor acts on the teacher's observation groups, which are added to the env after construction as the reference does, and
the student actor is regressed onto it (DAgger-only behaviour cloning; PPO-with-distillation raises in the reference too).

MI355X-first differences (same maths, pinned by tests/golden/ppo_v2.npz): as pbhc_amd/agents/mh_ppo.py — no host
synchronisation inside an iteration, fused sample / bootstrap / GAE / loss / clip+AdamW kernels over flat parameter buffers,
the motion embedding computed once per forward for actor and critic, env observations written straight into the rollout slabs,
one flat RCCL gradient all-reduce per optimiser step when envs are sharded over ranks.

What it shares with MHPPO is agents/base.py; the RL rollout is agents/rollout.py.
"""
from __future__ import annotations

import torch

from .. import _lib
from .. import dist as pdist
from ..utils import resume
from . import fused_mlp, rollout
from .agent_modules import Actor, ActorCritic
from .base import FlatAdamView, OnDeviceAgent, _load_checkpoint, switch_on
from .modules import BaseModule, apply_cat, apply_into


class PPO(OnDeviceAgent):
    def __init__(self, env, config, log_dir=None, device="cpu"):
        super().__init__(env, config, log_dir, device)
        self.learn = self.learn_RL if not self.train_distill else self.learn_distill

    def _init_config(self):
        super()._init_config()
        c = self.config
        self.num_envs = self.env.config.num_envs
        self.learning_rate = c.learning_rate
        self.priv_reg_coef_schedual = c.priv_reg_coef_schedual
        self.counter = 0
        self.train_distill = c.get("teacher_model_path", None) is not None
        self.dagger_only = bool(c.get("dagger_only", False))
        self._init_symmetry(c.get("symmetry", None))
        if self.dagger_only != self.train_distill:
            # the reference: distillation without dagger_only raises NotImplementedError in _update_distill (ppo_mimic.py:724);
            # dagger_only without a teacher stores no values/log-probs and fails in _update_ppo
            raise NotImplementedError("ppo_mimic supports dagger_only=False without a teacher (RL) or dagger_only=True with teacher_model_path (distillation)")
        if self.train_distill:
            self._preprocess_teacher_config()
        if c.module_dict.get("actor", {}).get("type", "MLP") != "MLP" or c.module_dict.get("critic", {}).get("type", "MLP") != "MLP":
            raise NotImplementedError("MoEMLP actors/critics")
        self.dagger_update_freq = c.get("dagger_update_freq", 20)
        self.hist_encoding = False

    def _init_symmetry(self, sym):
        """algo.config.symmetry: {enable, coef} — the mirror-symmetry term of the RL update: coef * mean (mu(M_o o) - M_a sg(mu(o)))^2.
        Absent or `enable: false`: the update is the one without it, launch for launch."""
        self.symmetry = bool(sym is not None and sym.get("enable", False))
        self.symmetry_coef = float(sym.get("coef", 1.0)) if self.symmetry else 0.0
        if not self.symmetry:
            return
        if self.train_distill or self.dagger_only:
            raise NotImplementedError("algo.config.symmetry.enable with dagger_only / teacher_model_path: the distillation update regresses the student "
                                      "onto the teacher's actions and has no PPO step the symmetry term could join")
        lib_ = getattr(self.env, "_motion_lib", None)
        aug = getattr(lib_, "augmentation", None)
        if aug is None or not aug.mirror:
            raise _lib.PbhcError("algo.config.symmetry.enable needs robot.motion.augmentation.mirror: without mirrored variants in the library the "
                                 "policy never tracks the references the term would tie it to")
        if not hasattr(self.env, "mirror_rows"):
            raise _lib.PbhcError("algo.config.symmetry.enable needs the general-tracking env (env.mirror_maps / env.mirror_rows)")
        self.env.mirror_maps()                      # refuses here, by name, what has no mirror

    def _preprocess_teacher_config(self):
        """ppo_mimic.py:121-145: the teacher's actor / future-target observation groups are added to the env under `teacher_*` names and
        the teacher's module config is rewritten to read them."""
        from pathlib import Path

        from ..envs import env_config
        from ..utils.config import load_config

        tc = load_config(str(Path(self.config.teacher_model_path).parent / "config.yaml"))
        groups, _, _ = env_config.determine_obs_dim(tc)
        od = self.env.config.obs.obs_dict
        od["teacher_actor_obs"] = list(tc.obs.obs_dict["actor_obs"])
        od["teacher_future_motion_targets"] = list(tc.obs.obs_dict["future_motion_targets"])
        self.env.rebuild_observations()
        self.algo_obs_dim_dict = self.env.config.robot.algo_obs_dim_dict
        assert self.algo_obs_dim_dict["teacher_actor_obs"] == groups["actor_obs"] and self.algo_obs_dim_dict["teacher_future_motion_targets"] == groups["future_motion_targets"]
        md = tc.algo.config.module_dict
        swap = lambda dims: ["teacher_actor_obs" if x == "actor_obs" else x for x in dims]
        md.actor.input_dim = swap(list(md.actor.input_dim))
        md.critic.input_dim = swap(list(md.critic.input_dim))
        md.actor.motion_encoder.input_dim = ["teacher_future_motion_targets"]
        self.config.teacher_module_dict = md

    # ------------------------------------------------------------------------------------
    def _setup_models_and_optimizer(self):
        c = self.config
        if self.env.config.use_vec_reward:
            c.module_dict.critic["output_dim"][-1] = self.num_rew_fn
        if self.train_distill:
            self.teacher_actor = Actor(self.algo_obs_dim_dict, c.teacher_module_dict.actor, self.num_act).to(self.device)
            sd = torch.load(c.teacher_model_path, map_location=self.device, weights_only=True)
            self.teacher_actor.load_state_dict({k[len("actor_module."):]: v for k, v in sd["model_state_dict"].items() if k.startswith("actor_module.")}, strict=True)
            for p in self.teacher_actor.parameters():
                p.requires_grad = False
            self.teacher_actor.eval()
        self.alg = ActorCritic(self.algo_obs_dim_dict, c.module_dict, self.num_act, c.init_noise_std).to(self.device)
        if self.train_distill:
            self.alg.actor.history_encoder.load_state_dict(self.teacher_actor.history_encoder.state_dict())
            for p in self.alg.actor.history_encoder.parameters():
                p.requires_grad_(False)
        if self._dp:
            for p in self.alg.parameters():
                pdist.broadcast(p.data, src=0)
        self._flatten_parameters()

    def _flatten_parameters(self):
        """Flat fp32 buffers [main parameters | history-encoder parameters]: `self.optimizer` (AdamW over every parameter; the history
        encoder never has a gradient in the PPO step, so torch skips it) steps the first segment, `hist_encoder_optimizer` the second."""
        dev = self.device
        named = list(self.alg.named_parameters())
        if self.dagger_only:       # distillation: only the actor MLP and the motion encoder ever have a gradient (ppo_mimic.py:711-721)
            self._is_main = lambda n: n.startswith("actor_module.actor_module.") or n.startswith("actor_module.motion_encoder.")
        else:
            self._is_main = lambda n: not n.startswith("actor_module.history_encoder.")
        main = [(n, p) for n, p in named if self._is_main(n)]
        hist = [(n, p) for n, p in named if not self._is_main(n)]
        self._n_main = sum(p.numel() for _, p in main)
        self._n_hist = sum(p.numel() for _, p in hist)
        # four spare floats between the two segments (in every flat buffer, so that one offset serves them all): slot `_n_main` of the
        # GRADIENT buffer carries the minibatch KL mean through the data-parallel all-reduce of the main segment — one collective per
        # optimiser step, every rank then takes the same learning-rate branch (as MHPPO does, mh_ppo.py: `_gflat[na + nc]`)
        self._o_hist = self._n_main + 4
        n = self._o_hist + self._n_hist
        self._pflat = torch.zeros(n, device=dev)
        self._gflat = torch.zeros(n, device=dev)
        self._mflat = [torch.zeros(n, device=dev), torch.zeros(n, device=dev)]     # per optimiser (the hist segment of [0] stays unused)
        self._vflat = [torch.zeros(n, device=dev), torch.zeros(n, device=dev)]
        self._slice_of = {}
        o = 0
        for nme, p in main + hist:
            if hist and p is hist[0][1]:
                o = self._o_hist
            k = p.numel()
            self._pflat[o:o + k].copy_(p.data.reshape(-1))
            p.data = self._pflat[o:o + k].view_as(p)
            p.grad = self._gflat[o:o + k].view_as(p)
            self._slice_of[nme] = (o, k, tuple(p.shape))
            o += k
        self._std_slice = self._slice_of["std"][:2]
        self._lr = torch.full((2,), float(self.learning_rate), device=dev)          # [0] is THE learning rate (the loss kernel adapts both)
        self._lr_hist = torch.full((1,), float(self.learning_rate), device=dev)     # hist_encoder_optimizer keeps its initial lr (ppo_mimic.py:184)
        self._adam_step = torch.zeros(2, device=dev)
        self._adam_scratch = torch.zeros(2, 512, dtype=torch.float64, device=dev)
        self._grad_norms = torch.zeros(2, device=dev)
        self._loss_scalars = torch.zeros(4, device=dev)
        self._g_sigma = torch.zeros(self.num_act, device=dev)
        self.betas, self.adam_eps, self.weight_decay = (0.9, 0.999), 1e-8, 0.01     # torch.optim.AdamW defaults
        # kept for checkpoint (de)serialisation in torch.optim.AdamW's format.  `optimizer`: AdamW over every parameter — distillation: over
        # the actor's (ppo_mimic.py:186-187) — of which only the main segment is ever stepped; `hist_encoder_optimizer`: the history encoder
        names = [n for n, _ in named if not self.dagger_only or n.startswith("actor_module.")]
        ent = lambda ns, live: [(*self._slice_of[n], live(n)) for n in ns]
        self.optimizer = FlatAdamView(self, ent(names, self._is_main), self._mflat[0], self._vflat[0], self._adam_step[0:1], self._lr, self.weight_decay)
        self.hist_encoder_optimizer = FlatAdamView(self, ent([n for n in names if n.startswith("actor_module.history_encoder.")], lambda n: True),
                                                   self._mflat[1], self._vflat[1], self._adam_step[1:2], self._lr_hist, self.weight_decay, load_lr=False)
        # every update zeroes its segment of `_gflat` before its backward: the MLP stacks may store their gradients into it directly
        self._direct_stacks = {"main": [], "hist": []}
        lo = self._gflat.data_ptr()
        for m in self.alg.modules():
            if isinstance(m, BaseModule):
                fused_mlp.grad_direct(m.module)
                off = (next(m.module.parameters()).grad.data_ptr() - lo) // 4
                self._direct_stacks["main" if off < self._n_main else "hist"].append(m.module)

    def _zero_grads(self, which):
        """zero one segment of the flat gradient buffer ("main": everything but the history encoder, "hist": the history encoder) and tell
        the declared stacks living in it that their next backward may store instead of accumulate"""
        (self._gflat[: self._n_main] if which == "main" else self._gflat[self._o_hist:]).zero_()
        for q in self._direct_stacks[which]:
            fused_mlp.grads_zeroed(q)

    def _setup_storage(self):
        S = len(self.env.tar_obs_steps)
        # ppo_mimic.py:206-216: the future targets of all S steps in one row
        self._obs_width = {k: d * S if k in ("future_motion_targets", "teacher_future_motion_targets") else d for k, d in self.algo_obs_dim_dict.items()}
        self._register_storage(self._obs_width, {"teacher_actions": self.num_act} if self.train_distill else {})
        if self.symmetry:
            dev, A = self.device, self.num_act
            self._grad_mu_m = torch.zeros(self._mb, A, device=dev)
            self._sym_scratch = torch.zeros(_lib.K["PBHC_SYM_MAX_BLOCKS"], device=dev)
            self._sym_scalar = torch.zeros(1, device=dev)

    def _eval_mode(self):
        self.alg.eval()

    def _train_mode(self):
        self.alg.train()

    # ---- checkpoints (ppo_mimic.py:237-265) --------------------------------------------------
    def load(self, ckpt_path):
        if ckpt_path is None:
            return None
        d = _load_checkpoint(ckpt_path, self.device)
        self.alg.load_state_dict(d["model_state_dict"])
        if self.load_optimizer:
            self.optimizer.load_state_dict(d["optimizer_state_dict"])
            self.learning_rate = d["optimizer_state_dict"]["param_groups"][0]["lr"]
            self.set_learning_rate(self.learning_rate)
        self.current_learning_iteration = d["iter"]
        self._restore_training_state(d)
        return d["infos"]

    def save(self, path, infos=None):
        torch.save(self._with_training_state({"model_state_dict": self.alg.state_dict(), "optimizer_state_dict": self.optimizer.state_dict(),
                                              "iter": self.current_learning_iteration, "infos": infos}), path)

    def _extra_training_state(self):
        """`counter` (it drives the priv_reg_coef schedule) and what the reference's dictionary leaves out of the second optimiser: the history
        encoder's Adam moments, its step count and its learning rate (`hist_encoder_optimizer` is in no checkpoint entry)"""
        o = self._o_hist
        return {"counter": int(self.counter), "hist_exp_avg": self._mflat[1][o:].clone(), "hist_exp_avg_sq": self._vflat[1][o:].clone(),
                "hist_adam_step": self._adam_step[1:2].clone(), "hist_lr": self._lr_hist.clone()}

    def _check_extra_training_state(self, extra):
        o = self._o_hist
        resume.check_tensors("PPO.load_training_state", extra, {"hist_exp_avg": self._mflat[1][o:], "hist_exp_avg_sq": self._vflat[1][o:]})

    def _load_extra_training_state(self, extra):
        o = self._o_hist
        self.counter = int(extra["counter"])
        resume.restore(extra, {"hist_exp_avg": self._mflat[1][o:], "hist_exp_avg_sq": self._vflat[1][o:], "hist_adam_step": self._adam_step[1:2],
                               "hist_lr": self._lr_hist})

    def set_learning_rate(self, learning_rate):
        self.learning_rate = learning_rate
        self._lr[:] = float(learning_rate)

    def update_counter(self):
        self.counter += 1

    # ---- learn loop (ppo_mimic.py:267-311) ---------------------------------------------------
    def learn_RL(self, num_iterations=None):
        def train():
            loss_dict = self._training_step()
            return self._training_step_dagger() if self.hist_encoding else loss_dict

        def before(it):
            self.hist_encoding = it % self.dagger_update_freq == 0

        self._learn_loop(num_iterations, self._rollout_step, train, before)

    # ---- distillation (ppo_mimic.py:313-357,533-549,711-724) ----------------------------------
    def learn_distill(self, num_iterations=None):
        def before(it):
            self.hist_encoding = True

        self._learn_loop(num_iterations, self._rollout_step_distill, self._training_step_distill, before)

    def teacher_actor_act_step(self, obs_dict, hist_encoding=True):
        return self.teacher_actor(obs_dict, hist_encoding, obs_key="teacher_actor_obs", target_key="teacher_future_motion_targets")

    def _rollout_step_distill(self, obs_dict):
        """DAgger-only rollout: the student acts with its mean on the history latent, the teacher's actions are recorded."""
        st, env, lib = self.storage, self.env, _lib.lib()
        T, N, R = self.num_steps_per_env, env.num_envs, self.num_rew_fn
        keys = list(self._obs_width.keys())
        stream = _lib.current_stream()
        with torch.inference_mode():
            for k in keys:
                getattr(st, k)[0].copy_(obs_dict[k])
            for t in range(T):
                b = {k: getattr(st, k)[t] for k in keys}
                st.teacher_actions[t].copy_(self.teacher_actor_act_step(b, hist_encoding=True))
                st.actions[t].copy_(self.alg.act_inference(b, hist_encoding=True))
                env.set_obs_outputs({k: getattr(st, k)[t + 1] for k in keys} if t + 1 < T else self._last_obs)
                nxt, rewards, dones, infos = env.step({"actions": st.actions[t]})
                _lib.check(lib.pbhc_rollout_post(rewards.data_ptr(), st.values[t].data_ptr(), dones.data_ptr(), infos["time_outs"].data_ptr(), N, R,
                                                 0.0, st.rewards[t].data_ptr(), st.dones[t].data_ptr(), self.cur_reward_sum.data_ptr(),
                                                 self.cur_episode_length.data_ptr(), self._ep_stats.data_ptr(), stream), "pbhc_rollout_post")
            st.step = T
            if self._dp and self._stat_mode == "rollout":
                self.env.sync_globals()                # sigma / curricula / log means: the mean over the ranks, once per rollout
            self._timer.split()
        return self._last_obs

    def _training_step_distill(self, indices=None):
        loss = {"bc_loss": torch.zeros((), device=self.device)}
        for batch in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs,
                                                       keys=["actor_obs", "future_motion_targets", "prop_history", "teacher_actions"], indices=indices):
            self._update_distill(batch, loss)
        n = self.num_learning_epochs * self.num_mini_batches
        self.storage.clear()
        out = {k: v / n for k, v in loss.items()}
        for k in ["Value", "Entropy", "Surrogate", "Actor_Load_Balancing_Loss", "Critic_Load_Balancing_Loss"]:
            out[k] = torch.zeros((), device=self.device)
        return out

    def _update_distill(self, b, loss):
        mu = self.alg.act_inference(b, hist_encoding=True)
        bc = (b["teacher_actions"] - mu).norm(p=2, dim=1).mean()
        self._zero_grads("main")
        bc.backward()
        if self._dp:
            pdist.allreduce_mean_(self._gflat[: self._n_main])
        self._adam(0, 0, self._n_main, self._lr[0:1])
        loss["bc_loss"] += bc.detach()
        return loss

    # ---- forward pieces ---------------------------------------------------------------------
    def _forward(self, b, hist_encoding, want_value=True):
        """mu, value (and the motion embedding computed ONCE for both; the reference encodes it twice with the same weights)."""
        a = self.alg.actor
        emb = a.motion_encoding(b["future_motion_targets"])
        latent = a.history_encoding(b["prop_history"]) if hist_encoding else a.priv_encoding(b["priv_obs"])
        # (the stacks read [observations | encoder outputs]: only the encoder columns carry a gradient — modules.apply_cat / apply_into)
        if "_xin_actor" in b and torch.is_grad_enabled():
            # the update: the observation columns of both stacks' inputs were laid out once, behind the minibatch shuffle (_assemble_inputs);
            # per optimiser step only the encoder outputs are copied in
            mu = apply_into(a.actor_module, b["_xin_actor"], b["actor_obs"].shape[1], [emb, latent])
            value = apply_into(self.alg.critic, b["_xin_critic"], b["actor_obs"].shape[1] + b["priv_obs"].shape[1], [emb]) if want_value else None
            return mu, value, latent
        mu = apply_cat(a.actor_module, b["actor_obs"], torch.cat([emb, latent], dim=-1))
        value = apply_cat(self.alg.critic, torch.cat([b["actor_obs"], b["priv_obs"]], dim=-1), emb) if want_value else None
        return mu, value, latent

    def _assemble_inputs(self, shuffled):
        """once per update, on the shuffled [T * N, C] tensors: the actor's and the critic's first-layer inputs with their observation columns in
        place — [actor_obs | (motion embedding, latent)] and [actor_obs | priv_obs | (motion embedding)] — so that an optimiser step copies 19 + 13 MB
        of encoder outputs where four `torch.cat` moved 110 MB (PBHC_ASSEMBLE_INPUTS=0: the concatenations)"""
        if not switch_on("PBHC_ASSEMBLE_INPUTS") or not all(k in shuffled for k in ("actor_obs", "priv_obs")):
            return
        a = self.alg.actor
        ao, po = shuffled["actor_obs"], shuffled["priv_obs"]
        if not (isinstance(a.actor_module, BaseModule) and a.actor_module._fused and isinstance(self.alg.critic, BaseModule) and self.alg.critic._fused and ao.is_cuda):
            return
        rows, wa, wp = ao.shape[0], ao.shape[1], po.shape[1]
        ka, kc = a.actor_module.module[0].in_features, self.alg.critic.module[0].in_features
        bufs = self.__dict__.get("_xin")
        if bufs is None or bufs[0].shape != (rows, ka) or bufs[1].shape != (rows, kc) or bufs[0].device != ao.device:
            bufs = self._xin = (torch.empty(rows, ka, device=ao.device), torch.empty(rows, kc, device=ao.device))
        bufs[0][:, :wa].copy_(ao)
        bufs[1][:, :wa].copy_(ao)
        bufs[1][:, wa:wa + wp].copy_(po)
        shuffled["_xin_actor"], shuffled["_xin_critic"] = bufs

    MIRRORED_KEYS = ("actor_obs", "future_motion_targets", "priv_obs")

    def _on_gather(self, shuffled):
        self._assemble_inputs(shuffled)
        if self.symmetry:
            self._mirror_inputs(shuffled)

    def _mirror_inputs(self, shuffled):
        """once per update, on the shuffled [T * N, C] tensors: ONE launch mirrors the three groups the actor reads on the RL path.  The mirrored
        actor_obs goes straight into the observation columns of a second assembled actor input (`_xin_actor_m`: both applications of the actor
        stack are alive until the backward, so they cannot share one); without assembled inputs, into a plain tensor for `apply_cat`."""
        bufs = self.__dict__.get("_mirrored")
        rows = shuffled["actor_obs"].shape[0]
        dev = shuffled["actor_obs"].device
        if bufs is None or bufs["future_motion_targets"].shape[0] != rows:
            bufs = self._mirrored = {k: torch.empty(rows, shuffled[k].shape[1], device=dev) for k in self.MIRRORED_KEYS[1:]}
        jobs = [(k, shuffled[k], bufs[k]) for k in self.MIRRORED_KEYS[1:]]
        if "_xin_actor" in shuffled:
            xm = self.__dict__.get("_xin_m")
            if xm is None or xm.shape != shuffled["_xin_actor"].shape:
                xm = self._xin_m = torch.empty_like(shuffled["_xin_actor"])
            jobs.append(("actor_obs", shuffled["actor_obs"], xm))
            shuffled["_xin_actor_m"] = xm
        else:
            if "actor_obs" not in bufs or bufs["actor_obs"].shape[0] != rows:
                bufs["actor_obs"] = torch.empty(rows, shuffled["actor_obs"].shape[1], device=dev)
            jobs.append(("actor_obs", shuffled["actor_obs"], bufs["actor_obs"]))
            shuffled["_m_actor_obs"] = bufs["actor_obs"]
        self.env.mirror_rows(jobs)
        shuffled["_m_future_motion_targets"], shuffled["_m_priv_obs"] = bufs["future_motion_targets"], bufs["priv_obs"]

    def _forward_mirrored(self, b):
        """mu of the SAME actor on the mirrored inputs (motion encoder, privileged encoder, actor stack): the second live application of each"""
        a = self.alg.actor
        emb = a.motion_encoding(b["_m_future_motion_targets"])
        latent = a.priv_encoding(b["_m_priv_obs"])
        if "_xin_actor_m" in b:
            return apply_into(a.actor_module, b["_xin_actor_m"], b["actor_obs"].shape[1], [emb, latent])
        return apply_cat(a.actor_module, b["_m_actor_obs"], torch.cat([emb, latent], dim=-1))

    def _rollout_step(self, obs_dict):
        """ppo_mimic.py:371-438 through agents/rollout.py.  Per control step: encoders + actor (+ critic) forward, sampling, the fused env step,
        ONE bootstrap/done/episode-stat kernel.  The MLP stacks (actor, critic, privileged encoder; PBHC_STACK_NETS_V2=0: none) run as ONE launch
        each from packed weights; the actor stack reads [actor_obs | motion embedding | latent] as three column segments (no concatenated copy)
        and samples in its last epilogue.  The critic runs once after the loop on the motion embeddings the per-step forwards left in
        `_emb_buf` (PBHC_CRITIC_BATCHED=0: the critic stack inside every control step, the plain `_forward`)."""
        st, env, a = self.storage, self.env, self.alg.actor
        T, N, A = self.num_steps_per_env, env.num_envs, self.num_act
        keys = list(self._obs_width.keys())
        mode = bool(self.hist_encoding)                    # the captured forward depends on the latent source
        batched = rollout.critic_batched(env)
        with torch.inference_mode():
            sigma = self.__dict__.get("_sigma_buf")
            if sigma is None:
                sigma = self._sigma_buf = torch.empty(A, device=self.device)          # fixed address: the captured sampling kernel reads it
            sigma.copy_(self.alg.sigma())
            if batched and (self.__dict__.get("_emb_buf") is None or self._emb_buf.shape != (T + 1, N, a.motion_encoder.output_dim)):
                self._emb_buf = torch.zeros(T + 1, N, a.motion_encoder.output_dim, device=self.device)
            nets = (a.actor_module, a.priv_encoder) if batched else (a.actor_module, self.alg.critic, a.priv_encoder)
            a_seq = a.actor_module.module if isinstance(a.actor_module, BaseModule) else None
            P = lambda x: x.data_ptr()

            def forward(t):
                b = {k: getattr(st, k)[t] for k in keys}
                if not batched:
                    return self._forward(b, mode)[:2]
                emb = a.motion_encoder(b["future_motion_targets"], out=self._emb_buf[t])
                latent = a.history_encoding(b["prop_history"]) if mode else a.priv_encoding(b["priv_obs"])
                xs = [b["actor_obs"], emb, latent]
                if d.fuse_sample:
                    smp = dict(std=sigma, seed=self._sample_seed, counter=self._ctr0.data_ptr(), counter_offset=t, actions=st.actions[t],
                               action_mean=st.action_mean[t], action_sigma=st.action_sigma[t], logp=st.actions_log_prob[t])
                    # (the riders go with the launch that samples; the encoder and privileged-stack launches above carry none)
                    if fused_mlp.forward_cat_inference(a_seq, xs, sample=smp, riders=d.rider) is False:
                        raise _lib.PbhcError("pbhc_mlp_fwd_cat does not apply to this policy (PBHC_FUSED_SAMPLE=0)")
                    return st.action_mean[t], None
                mu = fused_mlp.forward_cat_inference(a_seq, xs) if any(q is a_seq for q in d.packed) else False
                return (a.actor_module(torch.cat(xs, dim=-1)) if mu is False else mu), None

            def critic_rows():
                self._emb_buf[T].copy_(a.motion_encoding(self._last_obs["future_motion_targets"]))
                rows = lambda k: st.with_tail(k).flatten(0, 1)
                return torch.cat([rows("actor_obs"), rows("priv_obs"), self._emb_buf.flatten(0, 1)], dim=-1)

            d = rollout.RolloutSpec(
                keys=keys, batched=batched, forward=forward, sigma=sigma, sample_stack=a_seq if batched else None, key_extra=(mode, batched),
                stacks=[m.module for m in nets if m is not None and isinstance(m, BaseModule) and m._fused] if switch_on("PBHC_STACK_NETS_V2") else [],
                encoders=[e for e in (a.motion_encoder, a.history_encoder if mode else None) if e is not None and hasattr(e, "prepare_inference")],
                graph_allowed=lambda: True, critic=self.alg.critic, critic_rows=critic_rows,
                sample_ptrs=lambda t: (P(st.actions[t]), P(st.action_mean[t]), P(st.action_sigma[t]), P(st.actions_log_prob[t]), None if batched else P(st.values[t])))
            return rollout.collect(self, d, obs_dict)

    def _critic_values(self, obs_dict):
        return self.alg.evaluate(obs_dict)

    # ---- updates (ppo_mimic.py:493-709) ------------------------------------------------------
    UPDATE_KEYS = ["actor_obs", "priv_obs", "future_motion_targets", "prop_history", "actions", "values", "advantages", "returns", "actions_log_prob",
                   "action_mean", "action_sigma"]

    METERS = ["Value", "Entropy", "Surrogate", "priv_reg_loss", "Actor_Load_Balancing_Loss", "Critic_Load_Balancing_Loss"]

    def _meter_names(self):
        """the meters an optimiser step adds to, then the two load-balancing meters (they stay zero: no mixture-of-experts stacks here);
        "Symmetry" exists only while algo.config.symmetry is on"""
        return self.METERS if not self.symmetry else self.METERS[:4] + ["Symmetry"] + self.METERS[4:]

    def _training_step(self, indices=None):
        names = self._meter_names()
        meters, loss = self._begin_meters(names, summed=len(names) - 2)
        for batch in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, keys=self.UPDATE_KEYS, indices=indices,
                                                       on_gather=self._on_gather):
            self._update_ppo(batch, loss)
        self.update_counter()
        self.learning_rate = self._lr[0:1]
        return self._end_meters(names, meters, loss)

    def _training_step_dagger(self, indices=None):
        loss = {"hist_latent_loss": torch.zeros((), device=self.device)}
        for batch in self.storage.mini_batch_generator(self.num_mini_batches, self.num_learning_epochs, keys=["priv_obs", "prop_history"], indices=indices):
            self._update_dagger(batch, loss)
        n = self.num_learning_epochs * self.num_mini_batches
        self.storage.clear()
        self.update_counter()
        return {k: v / n for k, v in loss.items()}

    def _adam(self, which, o, n, lr):
        _lib.check(_lib.lib().pbhc_adam_clip(self._pflat[o:o + n].data_ptr(), self._gflat[o:o + n].data_ptr(), self._mflat[which][o:o + n].data_ptr(),
                                             self._vflat[which][o:o + n].data_ptr(), n, lr.data_ptr(), self._adam_step[which:which + 1].data_ptr(),
                                             float(self.max_grad_norm), self.betas[0], self.betas[1], self.adam_eps, self.weight_decay,
                                             self._adam_scratch[which].data_ptr(), self._grad_norms[which:which + 1].data_ptr(), _lib.current_stream()), "pbhc_adam_clip")

    def _update_ppo(self, b, loss):
        lib = _lib.lib()
        alg = self.alg
        mu, value, priv_latent = self._forward(b, hist_encoding=False)
        mu_m = self._forward_mirrored(b) if self.symmetry else None
        with torch.no_grad():
            hist_latent = alg.actor.history_encoding(b["prop_history"])
        priv_reg = (priv_latent - hist_latent).norm(p=2, dim=1).mean()
        sch = self.priv_reg_coef_schedual
        stage = min(max(self.counter - sch[2], 0) / sch[3], 1)
        coef = stage * (sch[1] - sch[0]) + sch[0]
        B = mu.shape[0]
        if B != self._mb:
            raise _lib.PbhcError("minibatch size changed")
        sigma = alg.sigma().detach().contiguous()
        self._zero_grads("main")
        adapt = int(self.desired_kl is not None and self.schedule == "adaptive")
        flags = (adapt if not self._dp else 0) | 2                      # bit 1: the ppo_mimic KL form
        st = _lib.current_stream()
        _lib.check(lib.pbhc_ppo_loss(mu.data_ptr(), sigma.data_ptr(), value.data_ptr(), b["actions"].data_ptr(), b["actions_log_prob"].data_ptr(),
                                     b["action_mean"].data_ptr(), b["action_sigma"].data_ptr(), b["advantages"].data_ptr(), b["returns"].data_ptr(),
                                     b["values"].data_ptr(), B, self.num_act, self.num_rew_fn, float(self.clip_param), float(self.value_loss_coef),
                                     float(self.entropy_coef), int(self.use_clipped_value_loss), float(self.desired_kl or 0.0), flags,
                                     self._grad_mu.data_ptr(), self._grad_value.data_ptr(), self._g_sigma.data_ptr(), self._loss_scalars.data_ptr(),
                                     loss["_acc"].data_ptr() if "_acc" in loss else None, self._lr.data_ptr(), self._loss_scratch.data_ptr(), st), "pbhc_ppo_loss")
        heads, grads = [mu, value], [self._grad_mu, self._grad_value]
        if mu_m is not None:
            # the target M_a mu is detached: the gradient reaches the weights through the mirrored application only, and `_grad_mu` stays the PPO one
            index, sign = self.env.mirror_maps()["actions"]
            _lib.check(lib.pbhc_symmetry_loss(mu.data_ptr(), mu_m.data_ptr(), index.data_ptr(), sign.data_ptr(), B, self.num_act, self.symmetry_coef,
                                              self._grad_mu_m.data_ptr(), self._sym_scratch.data_ptr(), self._sym_scalar.data_ptr(),
                                              loss["Symmetry"].data_ptr() if "Symmetry" in loss else None, st), "pbhc_symmetry_loss")
            heads.append(mu_m)
            grads.append(self._grad_mu_m)
        if coef != 0.0:
            heads.append(priv_reg * coef)
            grads.append(torch.ones((), device=self.device))
        torch.autograd.backward(heads, grads)
        if alg.std.requires_grad:                                               # d sigma / d std of clamp(std, min, max)
            so, sn = self._std_slice
            std = alg.std.detach()
            self._gflat[so:so + sn] = self._g_sigma * ((std >= alg.min_sigma) & (std <= alg.max_sigma))
        if self._dp:
            # ONE all-reduce per optimiser step: the main segment's gradients and, in the slot behind them, this rank's minibatch KL mean —
            # averaged by the collective itself; the learning-rate rule (ppo_mimic.py:617-630) then runs on the all-rank KL as one launch
            nb = self._n_main + adapt
            if adapt:
                self._gflat[self._n_main:nb].copy_(self._loss_scalars[3:4])
            pdist.allreduce_mean_(self._gflat[:nb])
            if adapt:
                _lib.check(lib.pbhc_kl_lr_rule(self._lr.data_ptr(), 2, self._gflat[self._n_main:].data_ptr(), float(self.desired_kl), st), "pbhc_kl_lr_rule")
        self._adam(0, 0, self._n_main, self._lr[0:1])
        if "_acc" in loss:
            pass                                           # (summed by the loss kernel's finishing block)
        else:
            loss["Value"] += self._loss_scalars[1]; loss["Surrogate"] += self._loss_scalars[0]; loss["Entropy"] += self._loss_scalars[2]
        loss["priv_reg_loss"] += priv_reg.detach()
        return loss

    def _update_dagger(self, b, loss):
        a = self.alg.actor
        with torch.no_grad():
            priv_latent = a.priv_encoding(b["priv_obs"])
        hist_loss = (priv_latent - a.history_encoding(b["prop_history"])).norm(p=2, dim=1).mean()
        self._zero_grads("hist")
        hist_loss.backward()
        if self._dp:
            pdist.allreduce_mean_(self._gflat[self._o_hist:])
        self._adam(1, self._o_hist, self._n_hist, self._lr_hist)
        loss["hist_latent_loss"] += hist_loss.detach()
        return loss

    # ---- evaluation / export surface --------------------------------------------------------
    @property
    def inference_model(self):
        return {"actor": self.alg.actor}

    @torch.no_grad()
    def evaluate_policy_steps(self, Nsteps):
        self._eval_mode()
        self.env.set_is_evaluating()
        obs = self.env.reset_all()
        for _ in range(Nsteps):
            obs, _, _, _ = self.env.step({"actions": self.alg.act_inference(obs, hist_encoding=True)})
        return obs

    @torch.no_grad()
    def evaluate_library(self, **kw):
        """Score every unique clip of the motion library once under the current policy (env.library_sweep; **kw: its max_steps, sync_every,
        before_wave).  Leaves and returns `self.library_metrics`."""
        self._eval_mode()
        self.library_metrics = self.env.library_sweep(lambda obs: self.alg.act_inference(obs, hist_encoding=True), **kw)
        return self.library_metrics

    def evaluate_policy(self):
        if getattr(self.env, "save_motion", False):
            # the reference's recorder lives in LeggedRobotMotionTracking, which this agent's general-tracking env does not derive from
            raise NotImplementedError("env.config.save_motion with ppo_mimic.PPO: the reference records with the motion-tracking env and MHPPO only")
        return self.evaluate_policy_steps(int(self.env.max_episode_length))

    def _log_scalars(self, w, it):
        w.add_scalar("Loss/learning_rate", float(self._lr[0]), it)
        w.add_scalar("Policy/mean_noise_std", float(self.alg.std.detach().mean()), it)

    def _log_line(self, loss_dict):
        return ", ".join(f"{k} {float(v):.4f}" for k, v in loss_dict.items() if "Load_Balancing" not in k) + f"  lr {float(self._lr[0]):.2e}"
