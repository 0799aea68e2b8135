"""The on-device rollout of both agents (mh_ppo.py:270-342, ppo_mimic.py:371-438): T x (policy forward + sampling, fused env step writing the
next observations into the next rollout slab, done / episode-statistics kernel), then the critic over all slabs and the time-out bootstrap,
then GAE.  No host synchronisation.

Per control step the dependent chain is env step -> policy forward (+ sampling in its last epilogue) -> env step.  Everything else of a step
— the env step's one-workgroup reduction (sigma EMA, curricula, step counter) and the done / episode-statistics kernel — is 13 us of work that
only the NEXT env step needs.  Two forms:
  rider form (default; `rider_form`): both ride in the policy launch of the next step as extra workgroups behind the stack's (PbhcRider,
    pbhc_mlp_fwd_*_riders: the policy forward reads nothing they write — its sampler is keyed by a snapshot of the step counter), so the chain
    is step -> policy(+ riders) -> step on ONE queue with no branch, no event and no cross-queue edge; the last step's pair follows the loop
    as plain launches;
  branch form (PBHC_ROLLOUT_RIDERS=0, and whenever something else lives behind the reduction: the per-step statistics exchange, the clip /
    start collectors, a per-step critic, the separate sampling kernel): they run on a branch stream NEXT to the chain, which waits for the
    branch once per step, right before the next env step — two cross-queue edges per control step.
`agent._rollout_form` says which one ran.  The critic's values are consumed only
by the time-out bootstrap and by GAE, both after the rollout: evaluated ONCE over all T + 1 slabs (whole-chip GEMM tiles) they cost 1.5 ms,
against 24 x 85 us for per-step forwards that share the chip with the step -> actor chain.  The weights are constant over the rollout: the MLP
stacks an agent names run as ONE launch per step from a packed copy (pbhc_mlp_fwd), with the sampling kernel in that launch's last epilogue,
keyed by a snapshot of the step counter + the step index (the same keys pbhc_policy_sample forms from the live counter, without waiting for
the previous step's reduction).

ONE hipGraph holds the whole loop (fork / join edges instead of stream events and 4 dispatch gaps per step): the steps read the replay frame
from the device-side cursor, their addresses (rollout slabs) are fixed, and the env's host-side events (DR re-draw, motion resample) are
checked for the whole window before (`rollout_graph_safe`); a rollout that contains one, the first rollout (online GEMM selection must not
run inside a capture) or one that is being timed launch by launch runs the loop step by step with one captured forward per step.

Switches (agents/base.py): PBHC_ROLLOUT_GRAPH=0 the eager loop, PBHC_ROLLOUT_SPLIT=0 one stream, PBHC_CRITIC_BATCHED=0 the critic inside
every control step, PBHC_FUSED_SAMPLE=0 the separate sampling kernel, PBHC_FWD_GRAPHS=0 eager per-step forwards, PBHC_ROLLOUT_RIDERS=0 the
branch form.
"""
from __future__ import annotations

import dataclasses
import typing

import torch

from .. import _lib
from . import fused_mlp
from .base import switch_on


def capture_graphs(agent, bodies, what=None, restore=None):
    """Record every `body()` of `bodies` into a hipGraph of its own (one memory pool) on the agent's side stream; nothing executes.
    -> ([graph], [what the bodies returned]).  what: a failed capture is reported once as "<what> graph capture failed" and None is returned
    (None: the exception propagates); restore(): called afterwards either way — the host-side state the recorded calls advanced."""
    side = agent.__dict__.setdefault("_graph_stream", torch.cuda.Stream(device=agent.device))
    graphs, outs, pool = [], [], None
    try:
        torch.cuda.synchronize()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for body in bodies:
                g = torch.cuda.CUDAGraph()
                # thread_local: the RCCL watchdog thread polls its events while we capture; only this thread's calls are policed
                with torch.cuda.graph(g, pool=pool, stream=side, capture_error_mode="thread_local"):
                    outs.append(body())
                pool = g.pool() if pool is None else pool
                graphs.append(g)
        torch.cuda.current_stream().wait_stream(side)
    except Exception as e:                                   # noqa: BLE001 (whatever the capture objects to: report once, go on eagerly)
        if what is None:
            raise
        print(f"[pbhc] {what} graph capture failed ({type(e).__name__}: {e}); the {what} stays eager")
        return None
    finally:
        if restore is not None:
            restore()
    return graphs, outs


def forward_graphs(agent, eager, key):
    """The eager loop is launch-bound on the host (≈18 launches per control step): the forward of step t — reading the fixed rollout slab t
    and the in-place-updated flat weights — is captured once as a hipGraph per step index and replayed with one launch.  The first rollout
    of a forward variant `key` runs eagerly (GEMM selection happens there); PBHC_FWD_GRAPHS=0 keeps everything eager."""
    if not switch_on("PBHC_FWD_GRAPHS"):
        return eager
    seen = agent.__dict__.setdefault("_fwd_seen", set())
    if key not in seen:
        seen.add(key)
        return eager
    cache = agent.__dict__.setdefault("_fwd_graph_cache", {})
    if key not in cache:
        cache[key] = capture_graphs(agent, [lambda t=t: eager(t) for t in range(agent.num_steps_per_env)])
    graphs, outs = cache[key]

    def replay(t):
        graphs[t].replay()
        return outs[t]

    return replay


@dataclasses.dataclass
class RolloutSpec:
    """What an agent's rollout is made of.
    keys: the observation groups stored per step.  batched: the critic runs once after the loop: `critic` on critic_rows() -> [(T + 1) * N, C]
    input rows.  forward(t) -> (mu, value or None) of slab t; it may read `fuse_sample` / `packed`, which the driver fills in before the first
    call.  sigma: the [A] standard deviation at a fixed address.  sample_ptrs(t): the five output addresses of pbhc_policy_sample.
    graph_allowed(): may this form be one hipGraph (asked once `fuse_sample` is known).  stacks: MLP stacks (nn.Sequential) to run from packed
    weights.  encoders: modules with prepare_inference() / release_inference().  sample_stack: the stack whose last epilogue can sample (None:
    this form of the forward cannot).  key_extra: what else the captured forward depends on.  critic_step(t) -> values of slab t, run on the
    branch stream ahead of forward(t) (None: no per-step critic outside forward).  after_step(t, nxt): called after env.step of step t.
    early_fwd_graphs: build the per-step forward graphs before deciding on the rollout graph (MHPPO) rather than when the eager loop runs
    (ppo_mimic).  rider: filled in by the driver around forward(t) in the rider form — the `PbhcRider` the launch of forward(t) that SAMPLES
    has to carry (fused_mlp.forward_sample / forward_cat_inference `riders=`), None otherwise."""

    keys: list
    batched: bool
    forward: typing.Callable
    sigma: torch.Tensor
    sample_ptrs: typing.Callable
    graph_allowed: typing.Callable
    critic: typing.Callable
    critic_rows: typing.Callable
    stacks: typing.Sequence = ()
    encoders: typing.Sequence = ()
    sample_stack: typing.Any = None
    key_extra: tuple = ()
    critic_step: typing.Optional[typing.Callable] = None
    after_step: typing.Optional[typing.Callable] = None
    early_fwd_graphs: bool = False
    packed: list = dataclasses.field(default_factory=list, init=False)      # the stacks that did pack   } filled in by collect()
    fuse_sample: bool = dataclasses.field(default=False, init=False)        # sampling in the forward   }
    rider: typing.Any = dataclasses.field(default=None, init=False)         # riders of forward(t)      }


def split_streams(env):
    return switch_on("PBHC_ROLLOUT_SPLIT") and hasattr(env, "set_finalize_stream")


def critic_batched(env):
    return split_streams(env) and switch_on("PBHC_CRITIC_BATCHED")


def rider_form(env, d):
    """May the reduction and the book-keeping of a control step ride in the next step's policy launch?  Only if that launch does not read the
    live step counter (the fused sampler) and nothing else lives behind the reduction: no per-step statistics exchange between the ranks, no
    clip / start collectors (they run behind the reduction on the finalize stream), no per-step critic on the branch."""
    return (split_streams(env) and hasattr(env, "take_finalize_rider") and d.fuse_sample and env._totals is None and env._clip_window is None
            and env._start_window is None and d.critic_step is None and switch_on("PBHC_ROLLOUT_RIDERS"))


def collect(agent, d, obs_dict):
    """one rollout of `agent` as `d` (a RolloutSpec) describes it, from the observations `obs_dict`, through GAE -> the observations after it"""
    st, env, lib = agent.storage, agent.env, _lib.lib()
    T, N, A, R = agent.num_steps_per_env, env.num_envs, agent.num_act, agent.num_rew_fn
    keys, batched = d.keys, d.batched
    c = _lib.K["PBHC_G_STEP_COUNTER"]
    counter = env.globals[c:].data_ptr()
    P = lambda x: x.data_ptr()
    with torch.inference_mode():
        for k in keys:
            getattr(st, k)[0].copy_(obs_dict[k])
        split = split_streams(env)
        # packed BEFORE any graph is captured below — a capture records whichever kernels the forward launches
        d.packed = [q for q in d.stacks if fused_mlp.pack_stack(q)]
        for e in d.encoders:
            e.prepare_inference()                          # weights re-laid-out once per rollout, in place (the captured graph reads them)
        if batched and (agent.__dict__.get("_time_outs") is None or agent._time_outs.shape != (T, N, 1)):
            agent._time_outs = torch.zeros(T, N, 1, dtype=torch.bool, device=agent.device)
        try:
            d.fuse_sample = d.sample_stack is not None and any(q is d.sample_stack for q in d.packed) and switch_on("PBHC_FUSED_SAMPLE")
            if d.fuse_sample:
                if agent.__dict__.get("_ctr0") is None:
                    agent._ctr0 = torch.zeros(1, dtype=torch.float64, device=agent.device)
                env.wait_finalize()
                agent._ctr0.copy_(env.globals[c:c + 1])
            fuse_sample = d.fuse_sample
            riders = rider_form(env, d)
            agent._rollout_form = "riders" if riders else "branch"
            fwd_key = tuple(d.key_extra) + (bool(d.packed), fuse_sample)
            if riders:
                # a captured forward holds the riders' descriptors: the env's addresses and replay window (graph_key, read once the env has
                # picked up a new window: finalize_rider) belong to its key
                env.finalize_rider()
                fwd_key += ("riders", *env.graph_key())
                stale = [k for k in agent.__dict__.get("_fwd_graph_cache", {}) if isinstance(k, tuple) and "riders" in k and k != fwd_key]
                for k in stale:
                    del agent._fwd_graph_cache[k]
            cur, br = torch.cuda.current_stream(), agent._branch_stream
            use_br = (split and not riders) or d.critic_step is not None
            if riders:
                env.set_finalize_deferred(True)
            elif split:
                env.set_finalize_stream(br)
            post_done = [agent.__dict__.setdefault("_post_done", torch.cuda.Event())]      # (a cell: a capture swaps the event it used for a fresh one)
            # per-step device addresses, formed once (the host's share of a control step is what bounds the loop once the critic is out of it)
            sc = agent.__dict__.get("_step_ptrs")
            if sc is None or sc[0] is not st or sc[2] != batched:
                sc = (st, [dict(sample=d.sample_ptrs(t), post=(P(st.rewards[t]), P(st.dones[t])), values=P(st.values[t]),
                                tout=P(agent._time_outs[t]) if batched else None, act={"actions": st.actions[t]},
                                obs_out={k: getattr(st, k)[t + 1] for k in keys} if t + 1 < T else agent._last_obs) for t in range(T)], batched)
                agent._step_ptrs = sc
            steps = sc[1]
            sigma_p, sum_p, len_p, stat_p = d.sigma.data_ptr(), agent.cur_reward_sum.data_ptr(), agent.cur_episode_length.data_ptr(), agent._ep_stats.data_ptr()
            gamma, seed, br_h = float(agent.gamma), agent._sample_seed, br.cuda_stream

            def rider_of(t, fin=True):
                """what the sampling launch of forward(t) carries: the reduction (fin) and the book-keeping of step t - 1.  Every address in it
                is fixed (env-owned step outputs, rollout slabs): a captured forward may hold it."""
                if t == 0:
                    return None
                r, sp = (env.finalize_rider() if fin else _lib.PbhcRider()), steps[t - 1]
                r.rew, r.values, r.reset_buf, r.time_outs = P(env.rew_buf), None if batched else sp["values"], P(env.reset_buf), P(env.time_out_buf)
                r.rewards_out, r.dones_out = sp["post"]
                r.cur_reward_sum, r.cur_episode_length, r.ep_stats, r.time_outs_out = sum_p, len_p, stat_p, sp["tout"]
                r.N, r.R, r.gamma, r.has_post = N, R, gamma, 1
                return r

            def forward_riders(t, fin=True):
                d.rider = rider_of(t, fin)
                try:
                    return d.forward(t)
                finally:
                    d.rider = None

            def run_loop_riders(cur, forward):
                """step -> policy(+ riders) -> step on ONE stream: forward(t) carries the reduction and the book-keeping of step t - 1"""
                stream = cur.cuda_stream
                for t in range(T):
                    sp = steps[t]
                    if t == 0:
                        forward(t)
                    elif env.finalize_owed:
                        env.take_finalize_rider()             # (host-side mark: forward(t), captured or not, holds the descriptor)
                        forward(t)
                    else:
                        # something inside the last env.step (a motion resample resets every env) read the globals and flushed the reduction
                        # as a plain launch already: the book-keeping rider alone, outside any captured forward
                        forward_riders(t, fin=False)
                    env.set_obs_outputs(sp["obs_out"])
                    # terminate_when_dof_far: env.step launches the pre-pass of step t right here, AFTER forward(t) — behind the reduction of
                    # step t - 1 (a rider of forward(t)) that clears the flag the pre-pass sets, as in the branch form
                    nxt, rewards, dones, infos = env.step(sp["act"])
                    if d.after_step is not None:
                        d.after_step(t, nxt)
                # the last step's pair: plain launches on the same stream
                env.flush_finalize()
                sp = steps[T - 1]
                _lib.check(lib.pbhc_rollout_post2(P(env.rew_buf), None if batched else sp["values"], P(env.reset_buf), P(env.time_out_buf), N, R, gamma,
                                                  *sp["post"], sum_p, len_p, stat_p, sp["tout"], stream), "pbhc_rollout_post2")

            fwd_fn = forward_riders if riders else d.forward
            fwd = forward_graphs(agent, fwd_fn, fwd_key) if d.early_fwd_graphs else None
            critic_fwd = None if d.critic_step is None else forward_graphs(agent, d.critic_step, "critic")

            def run_loop(cur, forward):
                if riders:
                    return run_loop_riders(cur, forward)
                stream = cur.cuda_stream
                if use_br:
                    br.wait_stream(cur)
                for t in range(T):
                    sp = steps[t]
                    if critic_fwd is not None:
                        with torch.cuda.stream(br):
                            st.values[t].copy_(critic_fwd(t))
                    mu, value = forward(t)
                    if split and t > 0:
                        cur.wait_event(post_done[0])          # reduction + book-keeping kernel of step t-1 (13 us of work, issued ~60 us ago)
                        env.finalize_joined()
                    if not fuse_sample:
                        _lib.check(lib.pbhc_policy_sample(mu.data_ptr(), sigma_p, None if value is None else value.data_ptr(), N, A, R, seed, counter,
                                                          *sp["sample"], stream), "pbhc_policy_sample")
                    env.set_obs_outputs(sp["obs_out"])
                    nxt, rewards, dones, infos = env.step(sp["act"])
                    if d.after_step is not None:
                        d.after_step(t, nxt)
                    # (batched critic: values == NULL — the time-out bootstrap is added after the loop — and the step's time-out flags are kept)
                    post2 = lambda values, s: _lib.check(lib.pbhc_rollout_post2(rewards.data_ptr(), values, dones.data_ptr(), infos["time_outs"].data_ptr(), N, R, gamma,
                                                                                *sp["post"], sum_p, len_p, stat_p, sp["tout"], s), "pbhc_rollout_post2")
                    if split:
                        # branch: [reduction of step t, queued by env.step] -> done / episode-statistics kernel of step t (per-step critic: values[t]
                        # were produced earlier on this stream and the bootstrap is added here) -> critic of slab t+1 (next iteration)
                        post2(None if batched else sp["values"], br_h)
                        post_done[0].record(br)
                    elif critic_fwd is not None:              # one stream, the per-step critic beside it: joined around the book-keeping kernel
                        cur.wait_stream(br)
                        _lib.check(lib.pbhc_rollout_post(rewards.data_ptr(), sp["values"], dones.data_ptr(), infos["time_outs"].data_ptr(), N, R,
                                                         gamma, *sp["post"], sum_p, len_p, stat_p, stream), "pbhc_rollout_post")
                        br.wait_stream(cur)
                    else:
                        post2(sp["values"], stream)
                if use_br:
                    cur.wait_stream(br)

            graph_ok = (switch_on("PBHC_ROLLOUT_GRAPH") and split and d.graph_allowed() and agent.__dict__.get("_rollouts_here", 0) >= 1
                        and not agent.__dict__.get("_rollout_graph_failed", False) and hasattr(env, "rollout_graph_safe") and env.rollout_graph_safe(T))
            ran = False
            if graph_ok:
                env.simulator.use_device_cursor()      # (every time: host-side stepping in between hands the frame index over by value again)
                # everything a captured env step froze (env.graph_key), the rollout slabs and the form of the forward; ONE cached graph per agent
                key = (id(st), *env.graph_key(), T) + fwd_key
                gc = agent.__dict__.get("_rollout_graph")
                if gc is None or gc[0] != key:
                    gc = _capture_rollout(agent, key, lambda: run_loop(torch.cuda.current_stream(), fwd_fn), post_done)
                if gc is not None:
                    gc[1].replay()
                    env.after_graph_steps(T)
                    ran = True
            agent._rollout_used_graph = ran
            if not ran:
                run_loop(cur, fwd or forward_graphs(agent, fwd_fn, fwd_key))
            if riders:
                env.set_finalize_deferred(False)
            elif split:
                env.set_finalize_stream(None)
        finally:
            # (also when a step raises: a stack left marked valid would serve stale weights to every later no-grad forward)
            for q in d.packed:
                fused_mlp.release_stack(q)
            for e in d.encoders:
                e.release_inference()
        last_values = None
        if batched:
            # mh_ppo.py:286-305 / ppo_mimic.py:384-386,425-431 for all steps at once: values of every slab + the bootstrap values of GAE (slab T: the
            # observations after the last step) from one launch set, then rewards += gamma * values * time_outs
            vals = d.critic(d.critic_rows()).view(T + 1, N, R)
            st.values.copy_(vals[:T])
            st.rewards.addcmul_(st.values, agent._time_outs.to(torch.float32), value=gamma)
            last_values = vals[T]
        st.step = T
        # two counts, equal in a run that never resumes: `_rollouts_done` paces update_start_sampling and is part of the training state
        # (exact resume); `_rollouts_here` says "the loop has run eagerly once in THIS process" (the gate of the first capture) and is not
        agent._rollouts_done = agent.__dict__.get("_rollouts_done", 0) + 1
        agent._rollouts_here = agent.__dict__.get("_rollouts_here", 0) + 1
        if agent._dp and agent._stat_mode == "rollout":
            env.sync_globals()                     # sigma / curricula / log means: the mean over the ranks, once per rollout
        so = getattr(env, "_start", None)          # start_sampling: the fold (outside the graph: an all-reduce under data parallelism)
        if so is not None and so["sampling"] and agent._rollouts_done % so["update_every_rollouts"] == 0:
            env.update_start_sampling()
        agent._timer.split()
        agent._compute_returns(agent._last_obs, last_values=last_values)
    return agent._last_obs


def _capture_rollout(agent, key, loop, post_done):
    """record the rollout loop into one hipGraph (the caller replays it).  On any failure the agent stays on the eager loop for good."""
    def renew():
        # the loop's event was recorded INSIDE the capture: an edge of the graph now, not an event a later eager step may wait on
        post_done[0] = agent._post_done = torch.cuda.Event()

    with agent.env.graph_steps(renew_events=True):
        got = capture_graphs(agent, [loop], what="rollout", restore=renew)
    if got is None:
        agent._rollout_graph_failed = True
        agent._rollout_graph = None
        return None
    agent._rollout_graph = (key, got[0][0])
    return agent._rollout_graph
