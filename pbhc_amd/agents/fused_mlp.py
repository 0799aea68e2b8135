"""Training-time forward/backward of a Linear/activation stack (`BaseModule`, reference agents/modules/modules.py:47-63) arranged for
MI355X:

* hidden layers run on the fp32 matrix cores in `pbhc_linear_act_fwd` — bias + ELU / ReLU applied to the accumulators, no separate
  activation pass — and their input gradients in `pbhc_linear_dgrad_act`, which folds in the activation derivative of the layer below and
  the row-block column sums of its bias gradient (csrc/pbhc_gemm.hip: LDS-DMA staged, `v_mfma_f32_32x32x2_f32`).  `PBHC_FUSED_GEMM=0`
  returns to library GEMMs (hipBLASLt / rocBLAS through torch) + the `pbhc_act_bwd_bias` pass;
* weight gradients and the narrow output layer stay library GEMMs (split-K batched form below); a split-rows MFMA weight-gradient kernel
  (`pbhc_linear_wgrad`) exists and is pinned by tests, but measured 104-107 TFLOP/s against the library's 115-123 and is opt-in
  (`PBHC_FUSED_WGRAD=1`);
* weight / bias gradients are written by the GEMM (`out=`) and the fused kernel straight into the parameter's `.grad` — a view of
  the agent's flat gradient buffer — so autograd's per-parameter `grad += tmp` launches and temporaries disappear.  That store
  OVERWRITES, so it is opt-in: only a stack whose owner declared `grad_direct(seq)` — "I zero the gradient buffer before every backward"
  (the agents do) — takes it, and only while the stack has ONE live application; a stack applied twice in outstanding graphs, and
  every stack of user code, hands its gradients back to autograd, which accumulates as usual;
* ELU runs in place and its derivative is taken from the output (`y > 0 ? 1 : y + 1`), so pre-activations are not kept;
* every fused backward ends in ONE finishing launch (`pbhc_colsum_final`: bias gradients, the output layer's weight gradient, split-K partials);
  an owner that brackets several stacks' backwards with begin_deferred_finish() / finish_deferred() gets one for all of them, and may hand
  finish_deferred() the second stage of its loss (`pbhc_colsum_final_ppo_reduce`: one more workgroup of that launch, not a launch of its own).
  MHPPO's optimiser step is then 17 launches: 3 forward (each layer of the two stacks shares ONE launch — forward_pair: the wide layers on
  64 x 128 tiles, the 128-column layers with their output layers on 32 x 128), the loss's first stage, per stack the output layer's one-pass
  backward + 3 weight-gradient GEMMs and the wide layer's input gradient, ONE input-gradient launch for both 128-column layers, the finishing
  launch — which also leaves the gradient's sums of squares (finish_deferred(reduce, sqnorm=...)) — and Adam (PBHC_STEP_FINISH=0: 18, a
  gradient-norm launch of its own; PBHC_PAIR_WIDE=0: 19, the wide layers' forwards per stack; PBHC_PAIR_TAILS=0: 21, everything per stack).
Same arithmetic as autograd's (the column sums are two-stage fp32 in a fixed order); pinned by the update-parity tests.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _lib

_ACT_ID = {nn.ELU: 1, nn.SiLU: 2, nn.ReLU: 3}
FUSED_GEMM = os.environ.get("PBHC_FUSED_GEMM", "1") != "0"
_WGRAD_P = {tuple(int(v) for v in kv.split(":")[0].split("x")): int(kv.split(":")[1]) for kv in os.environ.get("PBHC_WGRAD_P", "").split(",") if kv}
FUSED_WGRAD = os.environ.get("PBHC_FUSED_WGRAD", "0") == "1"        # measured slower than the library's split-K form: opt-in


class _Live:
    """one per forward application of a stack, owned by its autograd context: alive while that graph can still run backward"""
    __slots__ = ("__weakref__",)


def grad_direct(seq, on=True):
    """Owner's declaration for `seq` (an nn.Sequential of Linear / activation): every parameter's `.grad` is a preallocated contiguous
    tensor that the owner zeroes before each backward, so the backward may store into it instead of returning gradients to autograd."""
    seq._grad_direct = bool(on)
    if not hasattr(seq, "_fused_live"):
        seq._fused_live = weakref.WeakSet()
        seq._fused_shared = False
        seq._zero_epoch, seq._stored_epoch = 0, -1


def grads_zeroed(seq):
    """The owner has just zeroed the gradient buffer behind `seq`'s `.grad`s: the NEXT backward through the stack may store (overwrite);
    any further backward before the next zeroing accumulates through autograd — two sequential backward() calls between two zeroings
    (an auxiliary loss, gradient accumulation) therefore add up, as they do for any other module."""
    seq._zero_epoch = getattr(seq, "_zero_epoch", 0) + 1


def supported(module_seq):
    layers = list(module_seq)
    lin = [m for m in layers if isinstance(m, nn.Linear)]
    acts = [m for m in layers if not isinstance(m, nn.Linear)]
    if not lin or len(layers) != 2 * len(lin) - 1 or not isinstance(layers[-1], nn.Linear):
        return False
    if any(type(a) not in _ACT_ID for a in acts) or len({type(a) for a in acts}) > 1:
        return False
    return not any(isinstance(a, nn.ELU) and a.alpha != 1.0 for a in acts)


def _wgrad(d, x, out, defer=None):
    """out[n, k] = d^T[n, B] x[B, k]: the split-rows MFMA kernel (`pbhc_linear_wgrad`) where its shape rules allow, else the library form.
    `defer`: a list; a split-K result's [P, n, k] partials are appended to it as (partials, out) instead of being summed here — the caller
    sums every deferred pair in its ONE finishing launch (pbhc_colsum_final)."""
    n, k = out.shape
    B = d.shape[0]
    if FUSED_GEMM and FUSED_WGRAD and d.is_cuda and d.dtype == torch.float32 and out.is_contiguous() and d.is_contiguous() and x.is_contiguous():
        lib = _lib.lib()
        P = lib.pbhc_linear_wgrad_parts(B, n, k)
        if P > 0:
            scratch = torch.empty(P * n * k, device=d.device)
            _lib.check(lib.pbhc_linear_wgrad(d.data_ptr(), x.data_ptr(), out.data_ptr(), scratch.data_ptr(), B, n, k, _lib.current_stream()), "pbhc_linear_wgrad")
            LAUNCHES[0] += 1
            return out
    return _wgrad_library(d, x, out, defer)


def _wgrad_library(d, x, out, defer=None):
    """out[n, k] = d^T[n, B] x[B, k].  With B (minibatch rows, 24 576) >> n, k the single GEMM has few output tiles and a very long K loop:
    rocBLAS / hipBLASLt run it on part of the chip (128 x 256: 53 us = 30 TFLOP/s on MI355X).  Split over P row chunks it is a batched GEMM that
    fills the 256 CUs, followed by a [P, n, k] sum (23 us for the same shape); measured with tools/wgrad_splitk_probe.py."""
    n, k = out.shape
    B = d.shape[0]
    nk = n * k
    # (chosen in the update itself — bench.py with PBHC_WGRAD_P — not in a back-to-back probe, whose operands are warm in L2: 512 x 380 8 -> 4 parts
    # -0.35 ms per update, 768 x 630 one GEMM -> 2 parts -0.30, 256 x 512 16 -> 32 and 128 x 512 8 -> 16 another -0.05.  Round 3, with the
    # partial images summed by the backward's one finishing launch instead of a torch.sum each: 512 x 768 one GEMM -> 4 parts and 768 x 630
    # 2 -> 8 parts, 29.3 -> 28.85 ms per update on one box (16 parts: slower again) — tools/probes/wgrad_parts_sweep.sh)
    P = 0 if n < 64 else 32 if nk <= 128 * 256 else 16 if nk <= 128 * 512 else 32 if nk <= 256 * 512 else 4 if nk <= 512 * 768 else 8
    if _WGRAD_P:                                       # measurement aid: PBHC_WGRAD_P="512x380:4,256x512:8"
        P = _WGRAD_P.get((n, k), P)
    LAUNCHES[0] += 1
    if P == 0 or B % P or B // P < 256:
        return torch.mm(d.t(), x, out=out)
    part = torch.bmm(d.view(P, B // P, n).transpose(1, 2), x.view(P, B // P, k))
    if defer is not None and out.is_contiguous():
        defer.append((part, out))                          # summed by the caller's finishing launch (one launch for the whole backward
        return out                                         # instead of one torch.sum per layer: 5 x 6 us per optimiser step)
    LAUNCHES[0] += 1
    return torch.sum(part, 0, out=out)


# ---- the backward's finishing launch, shared ----------------------------------------------------------------------------------------------
# Every fused backward ends in ONE `pbhc_colsum_final` (bias gradients, the output layer's weight gradient, split-K partials): a latency-bound
# launch of ~16 us.  An owner that runs several stacks' backwards back to back on one stream (MHPPO: critic, then actor) brackets them with
# begin_deferred_finish() / finish_deferred(): stacks whose gradients are STORED (grad_direct) then hand their jobs — and the scratch tensors
# the jobs read — to a pending list, and one launch per PBHC_MAX_COLSUM_JOBS jobs finishes them all.  Stacks that return gradients to autograd
# finish at once as before (autograd may consume their outputs right after backward returns).
_DEFER = {"on": False, "jobs": [], "keep": []}
# launches issued by this module's training-time forward / backward (native entries and library GEMMs alike), for an owner that records
# how many launches its optimiser step was (MHPPO._update_launches).  Bookkeeping kept by hand at the call sites, not read from the stream:
# a launch added here must be counted here; the kernel traces under profiles/ are the measurement.
LAUNCHES = [0]


def begin_deferred_finish():
    _DEFER["on"] = True


def _launch_jobs(job_list, st, reduce=None):
    """`reduce` (a PbhcPpoReduce): the loss's second stage rides in the last launch as one more workgroup (pbhc_colsum_final_ppo_reduce)"""
    MAXJ = _lib.K["PBHC_MAX_COLSUM_JOBS"]
    lib = _lib.lib()
    for k in range(0, max(len(job_list), 1), MAXJ):
        chunk = job_list[k:k + MAXJ]
        jobs = (_lib.PbhcColsumJob * MAXJ)()
        for j, (part, out, nrb, n) in zip(jobs, chunk):
            j.part, j.out, j.num_row_blocks, j.n = part, out, nrb, n
        if reduce is not None and k + MAXJ >= len(job_list):
            _lib.check(lib.pbhc_colsum_final_ppo_reduce(jobs, len(chunk), C.byref(reduce), st), "pbhc_colsum_final_ppo_reduce")
            LAUNCHES[0] += 1
        elif chunk:
            _lib.check(lib.pbhc_colsum_final(jobs, len(chunk), st), "pbhc_colsum_final")
            LAUNCHES[0] += 1


class StepSqnorm:
    """An owner's description of its flat gradient buffer for finish_deferred(reduce, sqnorm=...): two consecutive segments (actor
    [0, n0), critic [n0, n0 + n1) of `gflat`) and the two Adam step counters `step`.  The finishing launch then also leaves each segment's
    sum of squares as per-workgroup partials (`pbhc_colsum_final_ppo_reduce_sqnorm`) and advances the counters, and the optimiser pass
    needs no norm pass (`pbhc_adam_clip2_parts` on `plan.part_ptr` / `plan.nparts`).
    What the jobs of a finish cover, the ranges they leave uncovered (direct `torch.mm` weight gradients at small minibatches: squared by
    rider workgroups) and the slot counts depend only on where the jobs WRITE — (out, rows, n) per job, fixed `.grad` views — and are worked
    out once per such signature and kept with the ctypes arrays; the scratch addresses the jobs READ are not part of the key (they are the
    allocator's to choose) and are refreshed in the kept job array every step, which is the one loop `_launch_jobs` runs anyway.
    `misses` counts the plans built: one per distinct signature."""

    class Plan:
        __slots__ = ("jobs", "num_jobs", "sq", "part", "part_ptr", "nparts")

    def __init__(self, gflat, n0, n1, step):
        self.gflat, self.n, self.step = gflat, (int(n0), int(n1)), step
        self._plans = {}
        self.misses = 0

    def _uncovered(self, base, n, covered):
        """the complement, in [0, n) floats from address `base`, of the (address, floats) intervals that lie in it -> [(off, len)]"""
        iv = sorted(((a - base) // 4, (a - base) // 4 + k) for a, k in covered if base <= a < base + 4 * n)
        out, at = [], 0
        for lo, hi in iv:
            if lo > at:
                out.append((at, lo - at))
            at = max(at, hi)
        if at < n:
            out.append((at, n - at))
        return out

    def plan(self, job_list, reduce):
        """-> the Plan of this finish, or None where the export's range table is too small for it (the caller takes the norm pass)"""
        key = (tuple(j[1:] for j in job_list), reduce.grad_std, reduce.A, self.gflat.data_ptr())
        got = self._plans.get(key)
        if got is not None:
            if got:
                for j, job in zip(got.jobs, job_list):
                    j.part = job[0]
            return got or None
        self.misses += 1
        if len(self._plans) >= 8:
            self._plans.clear()
        lib = _lib.lib()
        covered = [(out, n) for _, out, _, n in job_list] + [(reduce.grad_std, reduce.A)]
        sq = _lib.PbhcSqnorm()
        sq.step = self.step.data_ptr()
        base = self.gflat.data_ptr()
        for s, n in enumerate(self.n):
            ranges = self._uncovered(base, n, covered)
            if len(ranges) > _lib.K["PBHC_SQ_MAX_RANGES"]:
                self._plans[key] = False
                return None
            g = sq.seg[s]
            g.base, g.n, g.num_ranges = base, n, len(ranges)
            for r, (off, ln) in enumerate(ranges):
                g.range_off[r], g.range_len[r] = off, ln
            base += 4 * n
        P = StepSqnorm.Plan()
        P.num_jobs = len(job_list)
        P.jobs = (_lib.PbhcColsumJob * max(P.num_jobs, 1))()
        for j, (part, out, nrb, n) in zip(P.jobs, job_list):
            j.part, j.out, j.num_row_blocks, j.n = part, out, nrb, n
        slots = (C.c_int32 * 2)()
        _lib.check(lib.pbhc_colsum_final_ppo_reduce_sqnorm_slots(P.jobs, P.num_jobs, C.byref(reduce), C.byref(sq), slots), "pbhc_colsum_final_ppo_reduce_sqnorm_slots")
        P.nparts = (int(slots[0]), int(slots[1]))
        P.part = torch.empty(P.nparts[0] + P.nparts[1], dtype=torch.float64, device=self.gflat.device)     # (every slot is written by every finish)
        P.part_ptr = (P.part.data_ptr(), P.part.data_ptr() + 8 * P.nparts[0])
        for s in (0, 1):
            sq.seg[s].part, sq.seg[s].part_cap = P.part_ptr[s], P.nparts[s]
        P.sq = sq
        self._plans[key] = P
        return P


def finish_deferred(reduce=None, sqnorm=None):
    """launch what the backwards since begin_deferred_finish() left pending (current stream = the stream those backwards ran on).
    reduce: the owner's PbhcPpoReduce — the loss's second stage, whose results nothing reads before the optimiser pass, as one more
    workgroup of this launch instead of a one-workgroup launch of its own between the loss and the backward.
    sqnorm (with reduce): the owner's StepSqnorm — the launch also leaves the gradient's sums of squares and advances the Adam step counters.
    -> the StepSqnorm.Plan that ran (its partials feed pbhc_adam_clip2_parts), or None: the finish ran without the squares"""
    _DEFER["on"] = False
    job_list, keep = _DEFER["jobs"], _DEFER["keep"]
    _DEFER["jobs"], _DEFER["keep"] = [], []
    plan = sqnorm.plan(job_list, reduce) if (sqnorm is not None and reduce is not None) else None
    if plan is not None:
        MAXJ = _lib.K["PBHC_MAX_COLSUM_JOBS"]
        _lib.check(_lib.lib().pbhc_colsum_final_ppo_reduce_sqnorm(plan.jobs, plan.num_jobs, C.byref(reduce), C.byref(plan.sq), _lib.current_stream()),
                   "pbhc_colsum_final_ppo_reduce_sqnorm")
        LAUNCHES[0] += max(1, (plan.num_jobs + MAXJ - 1) // MAXJ)
    elif job_list or reduce is not None:
        _launch_jobs(job_list, _lib.current_stream(), reduce)
    del keep
    return plan


# ---- launches two stacks can share ---------------------------------------------------------------------------------------------------------
# _FusedMLP's forward and backward are generators (_fwd_steps / _bwd_steps) that yield the GEMM launches of a stack's hidden layers as requests:
#   "fwd"      (x, w, bias, y, pre, M, N, K, act)                                          pbhc_linear_act_fwd
#   "fwd_out"  (x, w, bias, y, pre, M, N, K, act, w_out, b_out, NO, out)                   pbhc_linear_act_fwd_out
#   "dgrad"    (dy, w, saved, dx, scratch, M, N, K, act)                       -> rows     pbhc_linear_dgrad_act
# The 128-wide tail's are one to four rounds of 32-row tiles with a short K loop — prologue-, epilogue- and ramp-bound — and the wide layers'
# forwards are launches that each fill and drain the chip; the actor's and the critic's use the same kernel instantiation: _run_joint issues
# such a pair as ONE launch (`*_pair`: the same tile code on a shared grid, bit for bit the same results).  Pairing never changes the tile shape a layer
# runs on — the column-sum partials, and with them the bias gradients, depend on the tile height — so a pair is formed only where both single
# entries would choose the pair kernel's tiles themselves: 32 x 128 (_issue_pair) or 64 x 128 (_issue_pair_wide).
def _issue(kind, a):
    """one request through its own entry -> number of partial rows (None for the forward)"""
    lib, st = _lib.lib(), _lib.current_stream()
    LAUNCHES[0] += 1
    if kind == "fwd":
        _lib.check(lib.pbhc_linear_act_fwd(*a, st), "pbhc_linear_act_fwd")
        return None
    if kind == "fwd_out":
        _lib.check(lib.pbhc_linear_act_fwd_out(*a, st), "pbhc_linear_act_fwd_out")
        return None
    nb = C.c_int(0)
    _lib.check(lib.pbhc_linear_dgrad_act(*a[:5], C.byref(nb), *a[5:], st), "pbhc_linear_dgrad_act")
    return nb.value


def _pairable(kind, a):
    """would the single entry run this request on the 32-row tiles the tail pair kernels are built for?  The tile-choice rule lives in ONE
    place, csrc/pbhc_gemm.hip (pick_shape): the forward yields "fwd_out" only under the condition on which it calls that entry at all (an
    entry that always runs 32 x 128 tiles), and for the input gradient the library is asked."""
    if kind == "fwd_out":
        return True
    if kind == "fwd":
        return False
    M, N, K = a[5], a[6], a[7]
    return bool(_lib.lib().pbhc_linear_dgrad_act_pairable(M, N, K))


def _pairable_wide(kind, a):
    """would the single entry run this request — a hidden layer's forward — on 64 x 128 tiles of the LDS-DMA kernel (the library's answer,
    as above)?  The wide layers' input gradients are not paired: built, bit for bit, and measured slower (profiles/update_paired_wide.txt)."""
    if kind != "fwd":
        return False
    M, N, K = a[5], a[6], a[7]
    return bool(_lib.lib().pbhc_linear_act_fwd_pairable(M, N, K))


def _issue_pair(kind, a0, a1):
    lib, st = _lib.lib(), _lib.current_stream()
    LAUNCHES[0] += 1
    if kind == "fwd_out":
        _lib.check(lib.pbhc_linear_act_fwd_out_pair(*a0, *a1, st), "pbhc_linear_act_fwd_out_pair")
        return None, None
    nb0, nb1 = C.c_int(0), C.c_int(0)
    _lib.check(lib.pbhc_linear_dgrad_act_pair(*a0[:5], C.byref(nb0), *a0[5:], *a1[:5], C.byref(nb1), *a1[5:], st), "pbhc_linear_dgrad_act_pair")
    return nb0.value, nb1.value


def _issue_pair_wide(kind, a0, a1):
    """two "fwd" requests of wide layers as one launch on 64 x 128 tiles"""
    assert kind == "fwd"
    LAUNCHES[0] += 1
    _lib.check(_lib.lib().pbhc_linear_act_fwd_pair(*a0, *a1, _lib.current_stream()), "pbhc_linear_act_fwd_pair")
    return None, None


def _run_single(gen):
    """run a _fwd_steps / _bwd_steps generator to its end, every request through its own entry -> the generator's result"""
    try:
        req = next(gen)
        while True:
            req = gen.send(_issue(*req))
    except StopIteration as e:
        return e.value


def _run_joint(g0, g1, wide=True, formed=None):
    """Two stacks' generators side by side over all their requests.  A stack runs ahead, every request through its own entry, until it
    holds one that a pair kernel could take (g0 first: a stack's own launches keep their order, and where nothing pairs the launch order is
    that of two separate applications); while both hold such a request of the same kind it is issued once for both — the tails on 32-row
    tiles, and with `wide` the wide layers on 64-row tiles (their kinds are appended to `formed`) — else each through its own entry, a
    hidden layer's "fwd" before the other stack's tail.  -> (result of g0, result of g1)"""
    gens, res = (g0, g1), [None, None]

    def step(j, reply=None, first=False):                  # -> the generator's next request, or None once it has returned (result kept)
        try:
            return next(gens[j]) if first else gens[j].send(reply)
        except StopIteration as e:
            res[j] = e.value
            return None

    def candidate(req):                                    # the pair kernel that could take this request: "tail", "wide" or None
        if _pairable(*req):
            return "tail"
        return "wide" if wide and _pairable_wide(*req) else None

    FIRST, HELD, DONE = object(), object(), object()
    # todo[j]: the reply generator j is waiting for (HELD: its request has not been issued yet; DONE: it has returned)
    r, c, todo = [None, None], [None, None], [FIRST, FIRST]
    while todo[0] is not DONE or todo[1] is not DONE:
        for j in (0, 1):                                   # g0 takes its reply and runs ahead to its next candidate (or its end) before g1 moves
            if todo[j] is DONE or todo[j] is HELD:
                continue
            r[j] = step(j, first=True) if todo[j] is FIRST else step(j, todo[j])
            while r[j] is not None:
                c[j] = candidate(r[j])
                if c[j] is not None:
                    break
                r[j] = step(j, _issue(*r[j]))
            if r[j] is None:
                todo[j] = DONE
        live = [j for j in (0, 1) if todo[j] is not DONE]
        if len(live) == 2 and r[0][0] == r[1][0] and c[0] == c[1]:
            if c[0] == "tail":
                todo[0], todo[1] = _issue_pair(r[0][0], r[0][1], r[1][1])
            else:
                todo[0], todo[1] = _issue_pair_wide(r[0][0], r[0][1], r[1][1])
                if formed is not None:
                    formed.append(r[0][0])
        else:
            if len(live) == 2 and (r[0][0] == "fwd") != (r[1][0] == "fwd"):      # the other stack's tail request waits for its partner
                live = [j for j in live if r[j][0] == "fwd"]
            for j in (0, 1):
                if todo[j] is not DONE:
                    todo[j] = _issue(*r[j]) if j in live else HELD
    return res[0], res[1]


class _Sub:
    """a stack's share of a joint application's autograd context: what _fwd_steps leaves on `ctx` for _bwd_steps"""
    grad_cols = None


class _FusedMLPPair(torch.autograd.Function):
    """Two independent stacks (MHPPO's actor and critic) in one application, so that their launches can be paired:
    forward  ONE launch for both stacks' first layers, one for their second (`wide`: 64 x 128 tiles), ONE for both tails (last hidden layer
    + output layer);
    backward each stack's output-layer backward and library weight gradient of the 128-wide layer, ONE launch for both input gradients of
    that layer, then each stack's remaining chain as in _FusedMLP.  Same kernels on the same tiles: every result is bit for bit what two
    _FusedMLP applications give.  `formed`: a list that receives the kinds of the wide pairs issued."""

    @staticmethod
    def forward(ctx, x0, x1, seq0, seq1, wide, formed, *params):
        s0, s1 = _Sub(), _Sub()
        (out0, saved0), (out1, saved1) = _run_joint(_FusedMLP._fwd_steps(s0, x0, seq0), _FusedMLP._fwd_steps(s1, x1, seq1), wide, formed)
        ctx.subs, ctx.nsaved0, ctx.wide, ctx.formed = (s0, s1), len(saved0), wide, formed
        ctx.save_for_backward(*saved0, *saved1)
        return out0, out1

    @staticmethod
    def backward(ctx, dout0, dout1):
        s0, s1 = ctx.subs
        saved = ctx.saved_tensors
        # (stack 1 leads, as autograd runs the later of two separate nodes first)
        (dx1, flat1), (dx0, flat0) = _run_joint(_FusedMLP._bwd_steps(s1, saved[ctx.nsaved0:], dout1, ctx.needs_input_grad[1]),
                                                _FusedMLP._bwd_steps(s0, saved[:ctx.nsaved0], dout0, ctx.needs_input_grad[0]), ctx.wide, ctx.formed)
        return (dx0, dx1, None, None, None, None, *flat0, *flat1)


def forward_pair(seq0, x0, seq1, x1, wide=True, formed=None):
    """(seq0(x0), seq1(x1)) as ONE autograd node with the two stacks' 128-wide tails in paired launches, or None — nothing launched —
    where that does not apply and the caller applies each stack on its own: both must be fused ELU / ReLU stacks that store their
    gradients in place (grad_direct, no other live application), end in Linear(K, 128) - act - Linear(128, <= 32), and the rows must be
    in the range where 32 x 128 tiles are chosen for both layers of every pair.  wide: also pair the wide layers' launches wherever both
    stacks' run on 64 x 128 tiles (asked per launch: the hidden layers' forwards); formed: a list that receives the kinds of those pairs
    ("fwd") as they are issued."""
    if not (FUSED_GEMM and FWD_OUT and OUT_BWD and torch.is_grad_enabled()):
        return None
    B = x0.shape[0]
    if not (x1.shape[0] == B and 8192 <= B <= 32 * _lib.K["PBHC_ACT_MAX_BLOCKS"]):
        return None
    params = []
    for seq, x in ((seq0, x0), (seq1, x1)):
        lin = [m for m in seq if isinstance(m, nn.Linear)]
        if not (supported(seq) and len(lin) >= 2 and type(seq[1]) in (nn.ELU, nn.ReLU) and x.is_cuda and x.dim() == 2 and x.dtype == torch.float32
                and getattr(seq, "_grad_direct", False) and len(seq._fused_live) == 0
                and lin[-2].out_features == 128 and lin[-2].in_features >= 4 and lin[-1].out_features <= 32
                and all(l.weight.is_contiguous() and l.weight.requires_grad and l.bias is not None for l in lin)):
            return None
        for l in lin:
            params += [l.weight, l.bias]
    return _FusedMLPPair.apply(x0, x1, seq0, seq1, bool(wide), formed, *params)


class _FusedMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, seq, *params):
        ctx.grad_cols = None
        return _FusedMLP._fwd(ctx, x, seq)

    @staticmethod
    def _fwd(ctx, x, seq):
        out, saved = _run_single(_FusedMLP._fwd_steps(ctx, x, seq))
        ctx.save_for_backward(*saved)
        return out

    @staticmethod
    def _fwd_steps(ctx, x, seq):
        """The forward as a generator: it launches everything itself except the hidden layers' GEMMs — launches a second stack's could share a
        grid with — which it YIELDS as (kind, arguments) requests — `_run_single` issues each through its own entry, `_run_joint` pairs two stacks' requests.
        `ctx`: any object (the autograd context, or a stack's `_Sub` of a joint one).  Returns (output, tensors to save)."""
        lin = [m for m in seq if isinstance(m, nn.Linear)]
        act = _ACT_ID[type(seq[1])] if len(lin) > 1 else 0
        saved_in, saved_act = [], []
        h = x if x.is_contiguous() else x.contiguous()
        fused = FUSED_GEMM and act in (1, 2, 3) and h.is_cuda and h.dtype == torch.float32
        if fused:
            lib, st = _lib.lib(), _lib.current_stream()
        out = None
        for i, l in enumerate(lin):
            saved_in.append(h)
            if out is not None:                        # the output layer already ran in the epilogue of the layer below
                continue
            if fused and i < len(lin) - 1 and l.weight.is_contiguous():
                B = h.shape[0]
                z = torch.empty(B, l.out_features, device=h.device)
                pre = torch.empty_like(z) if act == 2 else None          # SiLU' needs the pre-activation; ELU' / ReLU' come from the output
                lo = lin[-1]
                if (FWD_OUT and i == len(lin) - 2 and l.out_features == 128 and lo.out_features <= 32 and l.in_features >= 4 and lo.weight.is_contiguous()
                        and 8192 <= B <= 32 * _lib.K["PBHC_ACT_MAX_BLOCKS"]):
                    # 32-row tiles hold whole 128-wide rows: the narrow output layer is applied to them while they are in LDS
                    out = torch.empty(B, lo.out_features, device=h.device)
                    yield ("fwd_out", (h.data_ptr(), l.weight.data_ptr(), l.bias.data_ptr() if l.bias is not None else None, z.data_ptr(),
                                       pre.data_ptr() if pre is not None else None, B, 128, l.in_features, act, lo.weight.data_ptr(),
                                       lo.bias.data_ptr() if lo.bias is not None else None, lo.out_features, out.data_ptr()))
                    h = z
                    saved_act.append(pre if pre is not None else h)
                    continue
                yield ("fwd", (h.data_ptr(), l.weight.data_ptr(), l.bias.data_ptr() if l.bias is not None else None, z.data_ptr(),
                               pre.data_ptr() if pre is not None else None, B, l.out_features, l.in_features, act))
                h = z
                saved_act.append(pre if pre is not None else h)
                continue
            z = torch.addmm(l.bias, h, l.weight.t())
            LAUNCHES[0] += 1 if (i == len(lin) - 1 or act == 0) else 2          # (the library GEMM, and the eager activation pass)
            if i == len(lin) - 1:
                out = z
            elif act == 1:
                h = F.elu_(z)
                saved_act.append(h)                    # ELU' from the output
            elif act == 3:
                h = F.relu_(z)
                saved_act.append(h)
            else:
                saved_act.append(z)                    # SiLU' needs the pre-activation
                h = F.silu(z)
        ctx.seq, ctx.act, ctx.n, ctx.fused = seq, act, len(lin), fused
        ctx.live = None
        if getattr(seq, "_grad_direct", False):
            ctx.live = _Live()
            seq._fused_live.add(ctx.live)
        return out, [*saved_in, *saved_act]

    @staticmethod
    def backward(ctx, dout):
        dx, flat = _FusedMLP._bwd(ctx, dout, ctx.needs_input_grad[0])
        return (dx, None, *flat)

    @staticmethod
    def _bwd(ctx, dout, need_dx):
        return _run_single(_FusedMLP._bwd_steps(ctx, ctx.saved_tensors, dout, need_dx))

    @staticmethod
    def _bwd_steps(ctx, saved, dout, need_dx):
        """-> (input gradient or None, [gw, gb] per layer in forward order).  `ctx.grad_cols = c0`: only the input columns [c0, in) carry a
        gradient (_FusedMLPCat) — the first layer's input-gradient GEMM runs on that column slice of its weight alone.
        A generator like _fwd_steps: the input-gradient GEMMs are yielded as requests, and the number of partial rows the launch leaves is
        sent back."""
        lib, st = _lib.lib(), _lib.current_stream()
        lin = [m for m in ctx.seq if isinstance(m, nn.Linear)]
        L = ctx.n
        ins, acts = saved[:L], saved[L:]
        d = dout.contiguous()
        B = d.shape[0]
        widths = [l.out_features for l in lin]
        MAXB = _lib.K["PBHC_ACT_MAX_BLOCKS"]
        scratch = torch.empty(MAXB * sum(widths), device=d.device)       # per-layer row-block column sums, finished by ONE launch below
        jobs = []                                                   # (part, out, row blocks, n): one per layer's bias gradient, + the output layer's
        deferred = []                                               # weight gradient, + the split-K partials of the hidden layers' weight gradients
        keep = [scratch]
        nb = C.c_int(0)
        ret_w = []
        off = 0
        # direct stores only for a declared stack with one live application; once two applications were outstanding together, every
        # backward of that batch accumulates through autograd (the first one's direct store would otherwise be overwritten by the second)
        seq = ctx.seq
        may_direct = False
        if ctx.live is not None:
            if len(seq._fused_live) > 1:
                seq._fused_shared = True
            may_direct = not seq._fused_shared and seq._stored_epoch != seq._zero_epoch      # the first backward since the owner's zeroing
            if may_direct:
                seq._stored_epoch = seq._zero_epoch
        offs = []
        for l in lin:
            offs.append(off)
            off += MAXB * l.out_features
        have_partials = False                     # the fused input-gradient GEMM of the layer above already left d = dz and its column sums
        for i in reversed(range(L)):
            l = lin[i]
            n = l.out_features
            direct = (may_direct and l.weight.requires_grad and l.bias.requires_grad and l.weight.grad is not None and l.weight.grad.is_contiguous()
                      and l.bias.grad is not None and l.bias.grad.is_contiguous())
            gb = l.bias.grad if direct else torch.empty(n, device=d.device)
            part = scratch[offs[i]:offs[i] + MAXB * n]
            k_in = l.in_features
            if (i == L - 1 and i > 0 and ctx.fused and OUT_BWD and l.weight.is_contiguous() and ins[i].is_contiguous()
                    and ((k_in in (128, 256) and 1 <= n <= 32) or (ctx.act in (1, 3) and 8 < n <= 32 and k_in in (64, 192)))):
                # the narrow output layer: weight / bias / input gradient and the activation backward of the layer below in ONE pass over the rows.
                # 128 / 256 inputs (every shipped stack): on the matrix cores, any activation, 1..32 outputs.  Other widths: the streaming form, ELU /
                # ReLU stacks with 9..32 outputs only (it measured slower than the four launches on SiLU stacks, whose derivative needs a second
                # row stream and an exp per element — 58 / 45 us for 29 / 1 outputs)
                # (`pbhc_linear_out_bwd`; autograd: two library launches of split-K for 0.14 GFLOP, a column sum, a GEMM and an activation pass)
                gw = l.weight.grad if direct else torch.empty(n, k_in, device=d.device)
                part_dw = torch.empty(MAXB * n * k_in, device=d.device)    # (a local: alive until the finishing launch below has been queued)
                dn = torch.empty(B, k_in, device=d.device)
                below = acts[i - 1]
                _lib.check(lib.pbhc_linear_out_bwd(d.data_ptr(), ins[i].data_ptr(), None if below.data_ptr() == ins[i].data_ptr() else below.data_ptr(),
                                                   l.weight.data_ptr(), B, n, k_in, ctx.act, dn.data_ptr(), part_dw.data_ptr(), part.data_ptr(),
                                                   scratch[offs[i - 1]:].data_ptr(), C.byref(nb), st), "pbhc_linear_out_bwd")
                LAUNCHES[0] += 1
                jobs.append((part.data_ptr(), gb.data_ptr(), nb.value, n))
                jobs.append((part_dw.data_ptr(), gw.data_ptr(), nb.value, n * k_in))
                keep += [part_dw, gw, gb]
                ret_w.append((None, None) if direct else (gw, gb))
                d = dn
                have_partials = True
                continue
            if not have_partials:
                _lib.check(lib.pbhc_act_bwd_partials(d.data_ptr(), acts[i].data_ptr() if i < L - 1 else None, B, n, ctx.act if i < L - 1 else 0, d.data_ptr(),
                                                     part.data_ptr(), C.byref(nb), st), "pbhc_act_bwd_partials")
                LAUNCHES[0] += 1
            jobs.append((part.data_ptr(), gb.data_ptr(), nb.value, n))
            keep.append(gb)
            room = deferred
            if direct:
                _wgrad(d, ins[i], l.weight.grad, room)
                ret_w.append((None, None))
            else:
                ret_w.append((_wgrad(d, ins[i], torch.empty(n, l.in_features, device=d.device), room), gb))
            have_partials = False
            if i > 0 and ctx.fused and l.weight.is_contiguous() and B <= 128 * MAXB:      # (row blocks of 128 at most: the column-sum scratch holds MAXB of them)
                # d_below = (d W) * act'(output of the layer below) + its row-block column sums, in the GEMM's epilogue
                k = l.in_features
                dn = torch.empty(B, k, device=d.device)
                nb.value = yield ("dgrad", (d.data_ptr(), l.weight.data_ptr(), acts[i - 1].data_ptr(), dn.data_ptr(), scratch[offs[i - 1]:].data_ptr(),
                                            B, k, n, ctx.act))
                d = dn
                have_partials = True
            elif i > 0 or need_dx:
                LAUNCHES[0] += 1
                d = d @ (l.weight if (i > 0 or ctx.grad_cols is None) else l.weight[:, ctx.grad_cols:])
        for part_w, out_w in deferred:                              # [P, n, k] partials -> the weight gradient: the same fixed-order column sum
            jobs.append((part_w.data_ptr(), out_w.data_ptr(), part_w.shape[0], out_w.numel()))
            keep += [part_w, out_w]
        if _DEFER["on"] and may_direct and all(gw is None for gw, _ in ret_w):
            _DEFER["jobs"] += jobs                                  # every gradient is stored in place: the owner's finish_deferred() launches
            _DEFER["keep"] += keep
        else:
            _launch_jobs(jobs, st)
        if ctx.live is not None:
            seq._fused_live.discard(ctx.live)
            ctx.live = None
            if len(seq._fused_live) == 0:
                seq._fused_shared = False
        dx = d if need_dx else None
        flat = []
        for gw, gbias in reversed(ret_w):
            flat += [gw, gbias]
        return dx, flat


class _FusedMLPCat(torch.autograd.Function):
    """The same stack applied to cat([x_const, x_grad], -1) where only `x_grad` carries a gradient — ppo_mimic's actor / critic stacks read
    [observations | encoder outputs] (ppo_mimic.py:596-630 via agent_modules.py:118-128): autograd's form computes the first layer's input
    gradient for EVERY input column (24 576 x 512 x ~700: 0.14 ms per stack and optimiser step) and CatBackward then throws the observation
    columns away.  Here the input-gradient GEMM runs on the weight's trailing columns alone and is returned for `x_grad` directly."""

    @staticmethod
    def forward(ctx, x_const, x_grad, seq, *params):
        ctx.grad_cols = x_const.shape[-1]
        return _FusedMLP._fwd(ctx, torch.cat([x_const, x_grad], dim=-1), seq)

    @staticmethod
    def backward(ctx, dout):
        dx, flat = _FusedMLP._bwd(ctx, dout, ctx.needs_input_grad[1])
        return (None, dx, None, *flat)


class _FusedMLPInto(torch.autograd.Function):
    """_FusedMLPCat without the concatenation: `xfull` [B, in] already holds the constant (observation) columns [0, c0) — written once per
    update, when the minibatch shuffle is done — and the gradient-carrying parts (encoder outputs) are copied into its columns [c0, in) here:
    19 + 13 MB of copies per optimiser step of the general-tracking update where the two `torch.cat` moved 46 + 46 MB.  `xfull` is the first
    layer's saved input: it must stay untouched until this application's backward has run (the agent rewrites a slice only when its minibatch
    comes round again, an epoch later)."""

    @staticmethod
    def forward(ctx, xfull, c0, nparts, seq, *rest):
        parts = rest[:nparts]
        o = c0
        for t in parts:
            xfull[:, o:o + t.shape[1]].copy_(t)
            o += t.shape[1]
        assert o == xfull.shape[1]
        ctx.grad_cols = c0
        ctx.part_widths = [t.shape[1] for t in parts]
        return _FusedMLP._fwd(ctx, xfull, seq)

    @staticmethod
    def backward(ctx, dout):
        need = any(ctx.needs_input_grad[4:4 + len(ctx.part_widths)])
        dx, flat = _FusedMLP._bwd(ctx, dout, need)
        dparts = [None] * len(ctx.part_widths) if dx is None else list(torch.split(dx, ctx.part_widths, dim=1))
        return (None, None, None, None, *dparts, *flat)


OUT_BWD = os.environ.get("PBHC_FUSED_OUT_BWD", "1") != "0"
FWD_OUT = os.environ.get("PBHC_FUSED_FWD_OUT", "1") != "0"
FUSED_STACK = os.environ.get("PBHC_FUSED_STACK", "1") != "0"
_STACK_MAX_ROWS = int(os.environ.get("PBHC_FUSED_STACK_MAX_ROWS", "16384"))


def pack_stack(seq):
    """Owner's declaration "the weights of `seq` stay as they are until release_stack()" (a rollout, an evaluation run): repacks them into
    the operand layout of `pbhc_mlp_fwd` (one launch per layer, ~1.5 / 3.8 MB) so that `forward_inference` can run the whole stack as ONE
    launch.  Returns False — and changes nothing — where the stack kernel does not apply."""
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    lib = _lib.lib()
    n = len(lin)
    if not (FUSED_GEMM and FUSED_STACK and 1 <= n <= _lib.K["PBHC_MLP_MAX_LAYERS"] and lin[0].weight.is_cuda and lin[0].weight.dtype == torch.float32
            and all(l.weight.is_contiguous() for l in lin) and supported(seq)):
        return False
    c = getattr(seq, "_pbhc_stack", None)
    sizes = [int(lib.pbhc_mlp_packed_floats(l.out_features, l.in_features)) for l in lin]
    if c is None or c["sizes"] != sizes or c["bufs"][0].device != lin[0].weight.device:
        dims = (C.c_int * (n + 1))(lin[0].in_features, *[l.out_features for l in lin])
        lds = int(lib.pbhc_mlp_fwd_lds_bytes(dims, n))
        if lds > 160 * 1024:
            return False
        bufs = [torch.empty(sz, device=lin[0].weight.device) for sz in sizes]       # allocated once: captured graphs keep reading these addresses
        c = dict(sizes=sizes, bufs=bufs, dims=dims, w=(C.c_void_p * n)(*[b.data_ptr() for b in bufs]), valid=False)
        seq._pbhc_stack = c
    st = _lib.current_stream()
    for l, buf in zip(lin, c["bufs"]):
        _lib.check(lib.pbhc_mlp_pack(l.weight.data_ptr(), l.out_features, l.in_features, buf.data_ptr(), st), "pbhc_mlp_pack")
    c["b"] = (C.c_void_p * n)(*[None if l.bias is None else l.bias.data_ptr() for l in lin])
    c["valid"] = True
    return True


def release_stack(seq):
    """the weights of `seq` may change again: `forward_inference` goes back to the layer-by-layer kernels"""
    c = getattr(seq, "_pbhc_stack", None)
    if c is not None:
        c["valid"] = False


def rows_readable(x, span):
    """every row of the 2-D view `x` can be READ `span` floats wide without leaving x's storage: the stack kernel's 16-byte pieces and the
    one-launch encoder's 16-float k-steps read past a row's last column; inside the row pitch for every row but the last, whose over-read
    must not be the first bytes behind the allocation (a column slice that ends where its storage ends)"""
    return x.storage_offset() + (x.shape[0] - 1) * x.stride(0) + span <= x.untyped_storage().nbytes() // x.element_size()


def _pieces_readable(x):
    """the stack kernel takes its 16-byte path only with a row pitch % 4 == 0: then the piece that straddles the row's end is read whole"""
    return x.stride(0) % 4 != 0 or rows_readable(x, (x.shape[1] + 3) // 4 * 4)


def forward_inference(seq, x):
    """No-grad forward of the same stack (the rollout's policy / critic evaluation).  Between pack_stack() and release_stack() — the owner's
    promise that the weights are constant — the WHOLE stack is one launch (`pbhc_mlp_fwd`: a workgroup carries 16 rows through every layer,
    activations stay in LDS — at the rollout's 4 096 rows the layer-by-layer chain is launch- and tail-bound); otherwise hidden layers go
    through `pbhc_linear_act_fwd` and the narrow output layer through the library.  Plain launches on the current stream, so either form can be captured in a hipGraph."""
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    act = _ACT_ID[type(seq[1])] if len(lin) > 1 else 0
    lib, st = _lib.lib(), _lib.current_stream()
    # a rollout slab is a [N, C] view of 128-byte-padded rows: read in place through the row pitch (no .contiguous() copy of the slab)
    pitched = (not x.is_contiguous() and x.dim() == 2 and x.stride(1) == 1 and x.stride(0) >= x.shape[1] and x.stride(0) % 4 == 0
               and x.data_ptr() % 16 == 0 and x.shape[1] >= 4 and len(lin) > 1 and _pieces_readable(x))
    h = x if (x.is_contiguous() or pitched) else x.contiguous()
    B = h.shape[0]
    c = getattr(seq, "_pbhc_stack", None)
    if c is not None and c["valid"] and B <= _STACK_MAX_ROWS:
        out = torch.empty(B, lin[-1].out_features, device=h.device)
        _lib.check(lib.pbhc_mlp_fwd(h.data_ptr(), h.stride(0), c["w"], c["b"], c["dims"], len(lin), act, out.data_ptr(), out.stride(0), B, st), "pbhc_mlp_fwd")
        return out
    for l in lin[:-1]:
        z = torch.empty(B, l.out_features, device=h.device)
        bias = l.bias.data_ptr() if l.bias is not None else None
        if h.is_contiguous():
            _lib.check(lib.pbhc_linear_act_fwd(h.data_ptr(), l.weight.data_ptr(), bias, z.data_ptr(), None, B, l.out_features, l.in_features, act, st),
                       "pbhc_linear_act_fwd")
        else:
            _lib.check(lib.pbhc_linear_act_fwd_strided(h.data_ptr(), h.stride(0), 0, l.weight.data_ptr(), bias, z.data_ptr(), None, l.out_features, 0, 1,
                                                       B, l.out_features, l.in_features, act, st), "pbhc_linear_act_fwd_strided")
        h = z
    return torch.addmm(lin[-1].bias, h, lin[-1].weight.t())


def forward_sample(seq, x, std, seed, counter, counter_offset, actions, action_mean, action_sigma, logp, riders=None):
    """The policy stack AND the rollout's sampling (mh_ppo.py:286-296: act(), log-prob, the buffer writes) as one launch
    (`pbhc_mlp_fwd_sample`); needs pack_stack(seq).  Returns False — nothing launched — where that does not apply (the caller then runs
    forward_inference + pbhc_policy_sample).  riders: a `PbhcRider` whose work runs as extra workgroups of the launch
    (`pbhc_mlp_fwd_sample_riders`: the previous control step's reduction and book-keeping, agents/rollout.py)."""
    c = getattr(seq, "_pbhc_stack", None)
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    B = x.shape[0]
    if not (c is not None and c["valid"] and B <= _STACK_MAX_ROWS and x.dim() == 2 and x.stride(1) == 1 and lin[-1].out_features <= 32 and _pieces_readable(x)
            and actions.is_contiguous() and action_mean.is_contiguous() and action_sigma.is_contiguous() and logp.is_contiguous()):
        return False
    smp = _lib.PbhcMlpSample()
    smp.std, smp.counter, smp.seed, smp.counter_offset = std.data_ptr(), counter, int(seed), int(counter_offset)
    smp.actions, smp.action_mean, smp.action_sigma, smp.logp = actions.data_ptr(), action_mean.data_ptr(), action_sigma.data_ptr(), logp.data_ptr()
    act = _ACT_ID[type(seq[1])] if len(lin) > 1 else 0
    if riders is not None:
        _lib.check(_lib.lib().pbhc_mlp_fwd_sample_riders(x.data_ptr(), x.stride(0), c["w"], c["b"], c["dims"], len(lin), act, B, C.byref(smp), C.byref(riders),
                                                         _lib.current_stream()), "pbhc_mlp_fwd_sample_riders")
        return True
    _lib.check(_lib.lib().pbhc_mlp_fwd_sample(x.data_ptr(), x.stride(0), c["w"], c["b"], c["dims"], len(lin), act, B, C.byref(smp), _lib.current_stream()),
               "pbhc_mlp_fwd_sample")
    return True


def forward_cat_inference(seq, xs, sample=None, riders=None):
    """No-grad forward of a packed stack on `torch.cat(xs, -1)` WITHOUT the concatenation (`pbhc_mlp_fwd_cat`: the stack kernel stages its 16
    input rows from up to three column segments — observation slab | encoder outputs), optionally with the rollout's sampling in the last
    layer's epilogue (`sample`: dict(std, seed, counter, counter_offset, actions, action_mean, action_sigma, logp), as forward_sample).
    Returns the output [B, out] (None with `sample`: the mean lands in action_mean), or False — nothing launched — where it does not apply.
    riders: as forward_sample's (`pbhc_mlp_fwd_cat_riders`)."""
    c = getattr(seq, "_pbhc_stack", None)
    lin = [m for m in seq if isinstance(m, nn.Linear)]
    B = xs[0].shape[0]
    if not (c is not None and c["valid"] and B <= _STACK_MAX_ROWS and 1 <= len(xs) <= _lib.K["PBHC_MLP_MAX_SEGS"]
            and all(x.dim() == 2 and x.stride(1) == 1 and x.shape[0] == B and x.dtype == torch.float32 and x.is_cuda and _pieces_readable(x) for x in xs)
            and sum(x.shape[1] for x in xs) == lin[0].in_features):
        return False
    if sample is not None and not (lin[-1].out_features <= 32 and all(sample[k].is_contiguous() for k in ("actions", "action_mean", "action_sigma", "logp"))):
        return False
    inp = _lib.PbhcMlpInput()
    for i, x in enumerate(xs):
        inp.x[i], inp.ld[i], inp.width[i] = x.data_ptr(), x.stride(0), x.shape[1]
    inp.nseg = len(xs)
    act = _ACT_ID[type(seq[1])] if len(lin) > 1 else 0
    smp_ref, out = None, None
    if sample is not None:
        smp = _lib.PbhcMlpSample()
        smp.std, smp.counter, smp.seed, smp.counter_offset = sample["std"].data_ptr(), sample["counter"], int(sample["seed"]), int(sample["counter_offset"])
        smp.actions, smp.action_mean, smp.action_sigma, smp.logp = (sample[k].data_ptr() for k in ("actions", "action_mean", "action_sigma", "logp"))
        smp_ref = C.byref(smp)
    else:
        out = torch.empty(B, lin[-1].out_features, device=xs[0].device)
    if riders is not None:
        _lib.check(_lib.lib().pbhc_mlp_fwd_cat_riders(C.byref(inp), c["w"], c["b"], c["dims"], len(lin), act, None if out is None else out.data_ptr(),
                                                      0 if out is None else out.stride(0), B, smp_ref, C.byref(riders), _lib.current_stream()),
                   "pbhc_mlp_fwd_cat_riders")
        return out if sample is None else None
    _lib.check(_lib.lib().pbhc_mlp_fwd_cat(C.byref(inp), c["w"], c["b"], c["dims"], len(lin), act, None if out is None else out.data_ptr(),
                                           0 if out is None else out.stride(0), B, smp_ref, _lib.current_stream()), "pbhc_mlp_fwd_cat")
    return out if sample is None else None


def forward_into(seq, xfull, c0, parts):
    """seq(xfull) after copying `parts` (tensors [B, w_i], the gradient-carrying inputs) into xfull[:, c0:] — see _FusedMLPInto"""
    params = []
    for m in seq:
        if isinstance(m, nn.Linear):
            params += [m.weight, m.bias]
    return _FusedMLPInto.apply(xfull, c0, len(parts), seq, *parts, *params)


def forward(seq, x):
    """seq: nn.Sequential of Linear / activation; x [B, in]."""
    params = []
    for m in seq:
        if isinstance(m, nn.Linear):
            params += [m.weight, m.bias]
    return _FusedMLP.apply(x, seq, *params)


def forward_cat(seq, x_const, x_grad):
    """seq(cat([x_const, x_grad], -1)) with the input gradient formed for `x_grad` only (see _FusedMLPCat)"""
    params = []
    for m in seq:
        if isinstance(m, nn.Linear):
            params += [m.weight, m.bias]
    return _FusedMLPCat.apply(x_const, x_grad, seq, *params)
