"""The optimiser step without a gradient-norm pass of its own: the backward's finishing launch that also leaves the sums of squares of what
it stores (`pbhc_colsum_final_ppo_reduce_sqnorm`), the optimiser pass on those partials (`pbhc_adam_clip2_parts`), the glue that plans the
slots and the uncovered ranges (`fused_mlp.StepSqnorm`) and MHPPO's step with `PBHC_STEP_FINISH=1` against `=0`.

What is bit for bit: every output of the finishing launch against `pbhc_colsum_final` / `pbhc_colsum_final_ppo_reduce` on the same inputs, and
the optimiser pass against `pbhc_adam_clip2` when it is handed that run's norm partials.  Both sides of these comparisons run the same
column-sum bodies and the same `k_adam_clip`: they pin what the squares add and that the pass on partials is `pbhc_adam_clip2`'s pass, not
the bodies themselves — those are held to float64 by tests/test_gpu_gemm.py::test_colsum_final_job_shapes and, for `k_adam_clip` with its
first loads ahead of the norm reduction, by tests/test_gpu_ppo_kernels.py and the float64 comparison below.  What is bounded: the sum of a segment's slots
against numpy float64 over the bytes left in the gradient buffer, relative error <= 1e-9 (the products are exact in double, at most 2^21
additions of at most 2^-53 relative each), and the optimiser pass against the float64 torch optimiser by the rule of
tests/test_gpu_ppo_kernels.py (imported, not restated)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_paired_tails import _ordinary_graph_rng_state  # noqa: F401  (module fixture: see there; this module builds agents too)
from tests.test_gpu_ppo_kernels import (ADAM_STEPS, B1, B2, CLIP, DEV, ENTROPY_COEF, EPS, MAX_NORM, SEG_NORMS, SEG_STEP0, VALUE_COEF, WEIGHT_DECAYS, _LOSS_KEYS, _Flat,
                                        _adam_data, _adam_reference, _compare_segment, _guarded, _lib, _loss_inputs, _tail_ok)

pytestmark = pytest.mark.gpu

LOSS_SHAPE = (13, 23, 21)
SQ_TOL = 1e-9


# ---- one finish, both ways -----------------------------------------------------------------------------------------------------------------
class _Finish:
    """A flat gradient buffer of two segments laid out from `items` (per segment a list of ("job", rows, n[, "unaligned"]) / ("gap", floats) /
    ("std",)), jobs whose outputs lie elsewhere (`outside`: (rows, n) each, and grad_std when no segment holds ("std",)), random partial rows,
    and the loss's partial rows of a small minibatch.  run(): the finish through the existing exports into one copy of every output and
    through pbhc_colsum_final_ppo_reduce_sqnorm into another."""

    def __init__(self, items0, items1, outside=(), seed=0):
        L, lib = _lib()
        self.L, self.lib = L, lib
        g = torch.Generator().manual_seed(1234 + seed)
        B, A, R = LOSS_SHAPE
        self.A = A
        self.inp = {k: v.to(DEV) for k, v in _loss_inputs(B, A, R)[0].items()}
        self.scratch = torch.zeros(lib.pbhc_ppo_loss_scratch_floats(B), device=DEV)
        gm, gv = _guarded(B * A), _guarded(B * R)
        npart = C.c_int(0)
        L.check(lib.pbhc_ppo_loss_partials(*[self.inp[k].data_ptr() for k in _LOSS_KEYS], B, A, R, CLIP, VALUE_COEF, 1, 0, gm.data_ptr(), gv.data_ptr(),
                                           self.scratch.data_ptr(), C.byref(npart), L.current_stream()), "pbhc_ppo_loss_partials")
        self.npart, self.B = npart.value, B
        self.jobs, self.n, self.parts = [], [], []           # jobs: (part, where, offset, rows, n); where: "flat" or the index of an outside buffer
        std_at, off = None, 0
        for items in (items0, items1):
            start = off
            for it in items:
                if it[0] == "gap":
                    off += it[1]
                elif it[0] == "std":
                    std_at, off = off, off + A
                else:
                    self.jobs.append((self._part(g, it[1], it[2], len(it) > 3), "flat", off, it[1], it[2]))
                    off += it[2]
            self.n.append(off - start)
        self.total = off
        self.std_at = std_at
        self.outside_n = [n for _, n in outside] + ([A] if std_at is None else [])
        for k, (rows, n) in enumerate(outside):
            self.jobs.append((self._part(g, rows, n, False), k, 0, rows, n))
        self.start = torch.randn(self.total, generator=g).to(DEV)        # what earlier launches left in the gradient buffer

    def _part(self, g, rows, n, unaligned):
        buf = torch.randn(rows * n + 1, generator=g).to(DEV)
        self.parts.append(buf)
        return buf[1:] if unaligned else buf[:rows * n]

    def _outputs(self):
        o = dict(flat=_guarded(self.total), scalars=_guarded(4), lr=_guarded(2), outside=[_guarded(n) for n in self.outside_n])
        o["flat"][:self.total] = self.start
        o["lr"][:2] = torch.tensor([1e-3, 5e-4])
        return o

    def _job_list(self, o):
        return [(p.data_ptr(), (o["flat"][off:] if where == "flat" else o["outside"][where]).data_ptr(), rows, n) for p, where, off, rows, n in self.jobs]

    def _reduce(self, o):
        red = self.L.PbhcPpoReduce()
        gs = o["flat"][self.std_at:] if self.std_at is not None else o["outside"][-1]
        red.scratch, red.std, red.grad_std, red.scalars, red.lr = self.scratch.data_ptr(), self.inp["std"].data_ptr(), gs.data_ptr(), o["scalars"].data_ptr(), o["lr"].data_ptr()
        red.scalars_acc = None
        red.num_partials, red.B, red.A, red.adapt_lr, red.entropy_coef, red.desired_kl = self.npart, self.B, self.A, 1, ENTROPY_COEF, 0.01
        return red

    def plan(self, o, step):
        from pbhc_amd.agents import fused_mlp

        self.sqn = fused_mlp.StepSqnorm(o["flat"], self.n[0], self.n[1], step)
        return self.sqn.plan(self._job_list(o), self._reduce(o))

    def run(self):
        """-> (outputs of the existing exports, outputs of the new one, its partial buffers (guarded), slot counts, step counters)"""
        from pbhc_amd.agents import fused_mlp

        L, lib = self.L, self.lib
        old, new = self._outputs(), self._outputs()
        fused_mlp._launch_jobs(self._job_list(old), L.current_stream(), self._reduce(old))
        step = torch.tensor([5.0, 41.0], device=DEV)
        red = self._reduce(new)
        plan = self.plan(new, step)
        assert plan is not None
        parts = [_guarded(k, dtype=torch.float64) for k in plan.nparts]
        for s in (0, 1):                                             # the plan's own buffers replaced by guarded ones of exactly the slot count
            plan.sq.seg[s].part, plan.sq.seg[s].part_cap = parts[s].data_ptr(), plan.nparts[s]
        L.check(lib.pbhc_colsum_final_ppo_reduce_sqnorm(plan.jobs, plan.num_jobs, C.byref(red), C.byref(plan.sq), L.current_stream()), "pbhc_colsum_final_ppo_reduce_sqnorm")
        torch.cuda.synchronize()
        return old, new, parts, plan.nparts, step

    def check(self, expect_ranges=None):
        old, new, parts, nparts, step = self.run()
        for k in ("flat", "scalars", "lr"):                          # (whole buffers: the sentinels behind every output too)
            assert torch.equal(old[k], new[k]), k
        for a, b in zip(old["outside"], new["outside"]):
            assert torch.equal(a, b)
        assert _tail_ok(new["flat"], self.total) and _tail_ok(new["scalars"], 4) and _tail_ok(new["lr"], 2)
        assert step.tolist() == [6.0, 42.0]
        if expect_ranges is not None:
            got = [[(g.range_off[r], g.range_len[r]) for r in range(g.num_ranges)] for g in (self.sqn.plan(self._job_list(new), self._reduce(new)).sq.seg[s] for s in (0, 1))]
            assert got == expect_ranges, got
        flat = new["flat"][:self.total].cpu().numpy().astype(np.float64)
        off = 0
        for s in (0, 1):
            assert _tail_ok(parts[s], nparts[s]), f"segment {s}: written beyond its {nparts[s]} slots"
            got = float(parts[s][:nparts[s]].cpu().numpy().sum(dtype=np.float64)) if nparts[s] else 0.0
            want = float(np.sum(flat[off:off + self.n[s]] ** 2))
            rel = abs(got - want) / want if want else abs(got)
            print(f"SQ segment {s}: n {self.n[s]} slots {nparts[s]} sum {got!r} numpy {want!r} rel {rel:.3e}")
            assert rel <= SQ_TOL
            off += self.n[s]
        return nparts


TALL_N = [1, 31, 32, 33, 128]


@pytest.mark.parametrize("rows", [1, 8, 9, 56, 57, 64, 65, 384, 1024])
def test_tall_jobs_bit_identical_and_squares(rows):
    """tall jobs of every column count in one finish, a gap of three floats between neighbours (outputs at odd 4-byte offsets, uncovered
    ranges of length 3); 1024 rows: the cap PBHC_ACT_MAX_BLOCKS"""
    L, _ = _lib()
    assert L.K["PBHC_ACT_MAX_BLOCKS"] == 1024
    seg0 = [("std",)] + [x for n in TALL_N[:3] for x in (("gap", 3), ("job", rows, n))]
    seg1 = [x for n in TALL_N[3:] for x in (("job", rows, n), ("gap", 3))]
    _Finish(seg0, seg1, seed=rows).check()


@pytest.mark.parametrize("P", [2, 7, 8, 9, 32])
def test_wide_jobs_bit_identical_and_squares(P):
    """wide jobs (few images, >= 4096 columns, a multiple of 4) in both segments, the second at an odd offset (the four scalar stores)"""
    _Finish([("job", P, 4096), ("std",), ("gap", 1)], [("job", P, 4100)], seed=100 + P).check()


def test_wide_job_with_unaligned_partials_takes_the_tall_form():
    _Finish([("std",), ("job", 8, 4096, "unaligned")], [("gap", 5), ("job", 3, 4100, "unaligned")], seed=7).check()


def test_reduce_alone_and_nothing_covered():
    """num_jobs == 0, grad_std outside the segments: the launch is the reduce and the riders, every float of both segments uncovered"""
    f = _Finish([("gap", 1027)], [("gap", 9001)], seed=8)
    nparts = f.check(expect_ranges=[[(0, 1027)], [(0, 9001)]])
    assert nparts == (1, 3)                                           # 4096 floats per rider workgroup


def test_jobs_outside_the_segments_have_no_slot():
    f = _Finish([("gap", 5)], [("std",), ("gap", 4)], outside=[(9, 33), (8, 4096)], seed=9)
    assert f.check(expect_ranges=[[(0, 5)], [(f.A, 4)]]) == (1, 2)


def test_all_covered_17_jobs_two_launches():
    """17 jobs: two launches, the slots numbered across them; nothing uncovered, no rider"""
    seg0 = [("std",)] + [("job", 57, 33)] * 8 + [("job", 8, 4096)]
    seg1 = [("job", 65, 31)] * 8
    nparts = _Finish(seg0, seg1, seed=10).check(expect_ranges=[[], []])
    assert nparts == (1 + 8 * 2 + 4, 8)


def test_interleaved_uncovered_ranges():
    """uncovered ranges of 1, 3, 4, 5 and 1027 floats between jobs, and one of 9000 floats that starts at an odd offset (only 4-byte aligned,
    three rider workgroups, a tail of its own)"""
    seg0 = [("gap", 1), ("job", 9, 33), ("gap", 3), ("job", 64, 32), ("gap", 4), ("std",), ("gap", 5), ("job", 2, 4096), ("gap", 1027)]
    seg1 = [("job", 57, 31), ("gap", 9000), ("job", 7, 4100)]
    f = _Finish(seg0, seg1, seed=11)
    assert (f.n[0] + 31) % 2 == 1
    o = 0
    want0 = []
    for it in seg0:
        k = it[1] if it[0] == "gap" else f.A if it[0] == "std" else it[2]
        if it[0] == "gap":
            want0.append((o, k))
        o += k
    f.check(expect_ranges=[want0, [(31, 9000)]])


def test_straddling_job_is_refused_and_launches_nothing():
    L, lib = _lib()
    f = _Finish([("std",), ("job", 9, 33)], [("gap", 7)], seed=12)
    f.n = [f.n[0] - 2, f.n[1] + 2]                                    # the job's last two floats now lie in the second segment
    new = f._outputs()
    before = new["flat"].clone()
    step = torch.tensor([5.0, 41.0], device=DEV)
    with pytest.raises(L.PbhcError):
        f.plan(new, step)                                             # (the slot query refuses)
    sq = L.PbhcSqnorm()
    part = _guarded(64, dtype=torch.float64)
    base = new["flat"].data_ptr()
    for s in (0, 1):
        sq.seg[s].base, sq.seg[s].n, sq.seg[s].part, sq.seg[s].part_cap, sq.seg[s].num_ranges = base, f.n[s], part[32 * s:].data_ptr(), 32, 0
        base += 4 * f.n[s]
    sq.step = step.data_ptr()
    jl = f._job_list(new)
    jobs = (L.PbhcColsumJob * 1)()
    jobs[0].part, jobs[0].out, jobs[0].num_row_blocks, jobs[0].n = jl[0]
    red = f._reduce(new)
    assert lib.pbhc_colsum_final_ppo_reduce_sqnorm(jobs, 1, C.byref(red), C.byref(sq), L.current_stream()) == L.K["PBHC_EINVAL"]
    torch.cuda.synchronize()
    assert torch.equal(new["flat"], before) and _tail_ok(part) and step.tolist() == [5.0, 41.0]


# ---- the optimiser pass on the finish's partials --------------------------------------------------------------------------------------------
def _squares_by_riders(fin, f, n0, n1):
    """the finishing launch (the reduce of `fin`, a _Finish) with no job on the flat gradient of `f` (a _Flat): both segments one uncovered
    range each -> (guarded partial buffers, nparts)"""
    L, lib = _lib()
    o = fin._outputs()
    red = fin._reduce(o)
    sq = L.PbhcSqnorm()
    nparts = [(n + L.K["PBHC_SQ_RANGE_FLOATS"] - 1) // L.K["PBHC_SQ_RANGE_FLOATS"] for n in (n0, n1)]
    parts = [_guarded(k, dtype=torch.float64) for k in nparts]
    base = f.buf["grad"].data_ptr()
    for s, n in enumerate((n0, n1)):
        g = sq.seg[s]
        g.base, g.n, g.part, g.part_cap, g.num_ranges = base, n, parts[s].data_ptr(), nparts[s], 1
        g.range_off[0], g.range_len[0] = 0, n
        base += 4 * n
    sq.step = f.step.data_ptr()
    slots = (C.c_int32 * 2)()
    L.check(lib.pbhc_colsum_final_ppo_reduce_sqnorm_slots(None, 0, C.byref(red), C.byref(sq), slots), "slots")
    assert list(slots) == nparts
    L.check(lib.pbhc_colsum_final_ppo_reduce_sqnorm(None, 0, C.byref(red), C.byref(sq), L.current_stream()), "pbhc_colsum_final_ppo_reduce_sqnorm")
    return parts, nparts


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("wd", WEIGHT_DECAYS, ids=["adam", "adamw"])
@pytest.mark.parametrize("sizes", [(1, 1), (3, 5), (1027, 4098)])
def test_adam_from_the_finish_partials(sizes, wd, zero_grad):
    """the cases and references of test_adam_clip2_two_segments (one segment clipped, one not, in every step).  f: squares by the finishing
    launch, then pbhc_adam_clip2_parts — against the float64 torch optimiser.  h: pbhc_adam_clip2.  c: pbhc_adam_clip2_parts on h's OWN norm
    partials — bit for bit h (the export runs pbhc_adam_clip2's optimiser pass, nothing else)."""
    L, lib = _lib()
    fin = _Finish([("gap", 1)], [("gap", 1)], seed=13)
    n0, n1 = sizes
    segs = [(n0, 0), (n1, 1)]
    refs = [(_adam_reference(n, k, wd, torch.float64), _adam_reference(n, k, wd, torch.float32)) for n, k in segs]
    f, h, c = _Flat(segs), _Flat(segs), _Flat(segs)
    hyper = (MAX_NORM, B1, B2, EPS, wd, zero_grad)
    for it in range(ADAM_STEPS):
        gr = torch.cat([_adam_data(n, k)[3][it] for n, k in segs])
        for x in (f, h, c):
            x.buf["grad"][:n0 + n1] = gr
        parts, nparts = _squares_by_riders(fin, f, n0, n1)
        L.check(lib.pbhc_adam_clip2_parts(*f.ptrs(), n0, n1, f.lr.data_ptr(), f.step.data_ptr(), *hyper, parts[0].data_ptr(), nparts[0], parts[1].data_ptr(), nparts[1],
                                          f.norm.data_ptr(), L.current_stream()), "pbhc_adam_clip2_parts")
        L.check(lib.pbhc_adam_clip2(*h.ptrs(), n0, n1, h.lr.data_ptr(), h.step.data_ptr(), *hyper, h.scratch.data_ptr(), h.norm.data_ptr(), L.current_stream()), "pbhc_adam_clip2")
        hparts = [min((n + 2047) // 2048, 512) for n in sizes]       # pbhc_adam_clip2's norm blocks: 256 threads x 8 floats, at most 512
        c.step.copy_(h.step)                                          # (the pass on partials does not advance the counters)
        L.check(lib.pbhc_adam_clip2_parts(*c.ptrs(), n0, n1, c.lr.data_ptr(), c.step.data_ptr(), *hyper, h.scratch.data_ptr(), hparts[0], h.scratch[512:].data_ptr(), hparts[1],
                                          c.norm.data_ptr(), L.current_stream()), "pbhc_adam_clip2_parts")
        torch.cuda.synchronize()
        assert all(_tail_ok(p, k) for p, k in zip(parts, nparts))
        for idx, (off, n) in enumerate(((0, n0), (n0, n1))):
            _compare_segment(f"finish-adam {sizes} wd={wd} zero_grad={zero_grad} step {it} segment {idx}", f, off, n, idx, refs[idx][0][it], refs[idx][1][it], zero_grad)
            assert (float(f.norm[idx]) > MAX_NORM) == (SEG_NORMS[it][idx] > MAX_NORM)
        assert f.step.tolist() == [SEG_STEP0[0] + it + 1.0, SEG_STEP0[1] + it + 1.0] and torch.equal(c.step, h.step)
        for key in ("param", "grad", "exp_avg", "exp_avg_sq"):
            assert torch.equal(c.buf[key], h.buf[key]), f"{key}: the pass on pbhc_adam_clip2's partials differs from pbhc_adam_clip2"
        assert torch.equal(c.norm, h.norm)
        assert f.tails_ok() and c.tails_ok() and _tail_ok(f.norm, 2) and _tail_ok(c.norm, 2)


# ---- MHPPO ---------------------------------------------------------------------------------------------------------------------------------
STATE = ("_pflat", "_mflat", "_vflat", "_lr", "_adam_step")


def _ordered(t):
    """float32 bits as integers in the order of the floats: a difference of 1 is the adjacent float"""
    i = t.contiguous().view(torch.int32).to(torch.int64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a, b):
    return int((_ordered(a) - _ordered(b)).abs().max())


def _two_steps(monkeypatch, num_envs, steps_per_env):
    """two optimiser steps on one minibatch of a walk rollout with PBHC_STEP_FINISH=1 and =0 from the same state (the helper pattern of
    tests/test_gpu_paired_wide.py) -> per setting: state and loss scalars, per-step gradient norms, forms and launch counts"""
    import bench
    from pbhc_amd.agents.mh_ppo import MHPPO
    from tests.helpers import build_hip_env

    for name in ("PBHC_PAIR_TAILS", "PBHC_PAIR_WIDE"):
        monkeypatch.delenv(name, raising=False)
    torch.manual_seed(7)
    cfg, env = build_hip_env("v1_g1_23dof_walk.yaml", num_envs, noise_off=False,
                             overrides={"algo.config.num_mini_batches": 1, "algo.config.num_steps_per_env": steps_per_env})
    algo = MHPPO(env=env, config=cfg.algo.config, log_dir=None, device="cuda:0")
    algo.setup()
    algo._train_mode()
    obs = env.reset_all()
    env.simulator.set_replay(*bench.make_replay_on_device(env, algo.num_steps_per_env + 2, seed=7))
    algo._rollout_step(obs)
    n = algo.storage.num_envs * algo.storage.num_transitions_per_env
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(3)).to("cuda:0")
    batch = next(iter(algo.storage.mini_batch_generator(algo.num_mini_batches, 1, keys=algo.UPDATE_KEYS, indices=perm)))
    batch = {k: v.clone() for k, v in batch.items()}
    assert batch["actor_obs"].shape[0] == num_envs * steps_per_env
    start = {k: getattr(algo, k).clone() for k in STATE}
    out = {}
    for setting in ("1", "0"):
        monkeypatch.setenv("PBHC_STEP_FINISH", setting)
        for k in STATE:
            getattr(algo, k).copy_(start[k])
        algo._gflat.zero_()
        algo._gflat_clean = False
        loss = {k: torch.zeros((), device="cuda:0") for k in algo.METERS}
        scalars, norms, forms, launches = [], [], [], []
        for _ in range(2):
            algo._update_ppo(batch, loss)
            scalars.append(algo._loss_scalars.clone())
            norms.append(algo._grad_norms.clone())
            forms.append((algo._update_form, algo._step_finish))
            launches.append(algo._update_launches)
        torch.cuda.synchronize()
        res = {k: getattr(algo, k).clone() for k in STATE}
        res["scalars"] = torch.stack(scalars)
        res["losses"] = torch.stack([loss[k] for k in ("Value", "Surrogate", "Entropy")])
        assert not algo._gflat.view(torch.int32).any()               # the pass left the gradient buffer zeroed
        if setting == "1":                                            # one plan for both steps: the second found the first's
            assert algo._sqnorm.misses == 1
        out[setting] = (res, torch.stack(norms), forms, launches)
    assert not torch.equal(out["1"][0]["_pflat"], start["_pflat"])
    return out


def _compare_settings(out, tag):
    (new, nn, _, _), (old, on, _, _) = out["1"], out["0"]
    d = _ulps(nn, on)
    print(f"STEP_FINISH {tag}: gradient norms {nn.tolist()} against {on.tolist()}: {'equal' if d == 0 else f'{d} ulp apart'}")
    assert d <= 1, "the gradient norms are neither equal nor adjacent floats"
    assert torch.equal(new["_adam_step"], old["_adam_step"]) and new["_adam_step"].tolist() == [2.0, 2.0]
    if d == 0:                                                        # the expected case: everything bit for bit
        for k in new:
            assert torch.equal(new[k], old[k]), k
    else:
        assert _ulps(new["_pflat"], old["_pflat"]) <= 1
        assert _ulps(new["_mflat"], old["_mflat"]) <= 8 and _ulps(new["_vflat"], old["_vflat"]) <= 8
        for k in ("_lr", "scalars", "losses"):                        # (the first step's loss does not depend on the norm at all; the second's does)
            assert torch.allclose(new[k], old[k], rtol=1e-5, atol=1e-7), k


@pytest.mark.parametrize("num_envs, launches", [(512, 18), (1024, 17)])
def test_mhppo_step_finish_every_hidden_dw_split(monkeypatch, num_envs, launches):
    """512 envs x 16 steps = 8192 rows: the paired form, every hidden layer's weight gradient split-K — every gradient element is written
    by the finishing launch, no rider.  At 8192 rows the second wide layers' forwards do not pair (the actor's runs on 64 x 64 tiles,
    tests/test_gpu_paired_wide.py), so a step is 18 launches against 19; from 16 384 rows (1024 envs) on — the benchmark's 24 576 among
    them — both pair and it is 17 against 18."""
    out = _two_steps(monkeypatch, num_envs, 16)
    assert out["1"][2] == [("paired", "squares")] * 2 and out["0"][2] == [("paired", "norm-pass")] * 2
    assert out["1"][3] == [launches] * 2 and out["0"][3] == [launches + 1] * 2
    _compare_settings(out, f"{num_envs * 16} rows")


def test_mhppo_step_finish_at_512_rows_rider_ranges(monkeypatch):
    """32 envs x 16 steps: no split-K (direct library weight gradients), so the hidden layers' weight gradients are uncovered ranges squared
    by the rider workgroups; one launch fewer than with the norm pass"""
    out = _two_steps(monkeypatch, 32, 16)
    assert [f[1] for f in out["1"][2]] == ["squares"] * 2 and [f[1] for f in out["0"][2]] == ["norm-pass"] * 2
    assert [a - b for a, b in zip(out["0"][3], out["1"][3])] == [1, 1]
    _compare_settings(out, "512 rows")
