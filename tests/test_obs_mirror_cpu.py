"""The observation mirror maps (pbhc_amd/envs/obs_mirror.py) on the CPU: shape and involution for the three v2 fixture configs, the refusals
by name, and equivariance against the oracle env — which is the authority on every sign.

Equivariance (`Mirrored`, shared with tests/test_gpu_symmetry.py).  An oracle motion library of two clips — a source and its float64-restated
mirror image (tests/test_motion_augment_cpu.restate) — and 2n envs: the first n track the source, the last n the mirror.  Everything the
second half is given — DR draws, replay frames (root state, joints, contact forces), actions — is the mirror image of the first half's, whose
replay frames are the reference plus a random perturbation, so that no difference term is zero.  After 12 steps (the history is full) and at
every step before, `obs[group][n:]` must be the group's map applied to `obs[group][:n]`.

Bounds, per element and from library data only.  For every reference quantity q (root position / rotation / velocity / angular velocity,
joint angles, body positions) delta_q = max |q(mirror clip) - M q(source clip)| over every time the test reads, M the physical mirror of that
quantity (a polar vector (x, -y, z), an axial one (-x, y, -z), a quaternion (-x, y, -z, w) up to its sign, joints permuted and signed).  An
element that depends on q is held to scale x delta_q + 3e-5 (abs + rel), scale the key's observation scale and 3e-5 the project's observation
tolerance; one that depends on two quantities (`REF_TOL`: a root velocity expressed in the root's frame) to the sum of their deltas.  The robot's
own state is mirrored exactly; a body-position element of ITS forward kinematics carries the skeleton's offset asymmetry a once per link of the
chain: (max depth + 2) a, as test_fk_of_the_mirrored_clip_is_the_mirrored_fk (the anchor it is taken relative to is body 0: the robot's root
state in x and y, the reference's root height in z, neither of which carries any).  Every delta is printed and capped, so that a wrong M cannot widen a bound unseen.  The clips
and start times are the ones whose frames lie inside a run on which the reference's finite-difference angular velocity IS mirror-symmetric
(the test asserts that precondition from the two lookups).
"""
import copy

import numpy as np
import pytest
import torch

from pbhc_amd import _lib
from pbhc_amd.envs import obs_mirror
from pbhc_amd.motion_augment import mirror_tables
from tests.helpers import build_env_config, fixture_config, skel_from_golden
from tests.test_motion_augment_cpu import CLIP29, load_clip, restate, skeleton

V2_CONFIGS = ["v2_g1_23dof_student.yaml", "v2_g1_23dof_teacher.yaml", "v2_g1_29dof_teacher.yaml"]


def _cpu_build(cfgname, mutate=None, overrides=None):
    return build_env_config(cfgname, overrides, num_envs=4, seed=0, general=True, has_contact_mask=True, mutate=mutate)


# ---- 1. involution and shape -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfgname", V2_CONFIGS)
def test_every_group_map_has_the_groups_width_and_is_an_involution(cfgname):
    cfg, skel, c, L = _cpu_build(cfgname)
    maps = obs_mirror.build(cfg, skel)
    assert set(maps) == set(cfg.obs.obs_dict) | {"actions"}
    for group, (index, sign) in maps.items():
        C = skel.num_dof if group == "actions" else L.group_dims[group]
        assert index.dtype == np.int32 and sign.dtype == np.float32 and index.shape == (C,) and sign.shape == (C,), group
        assert np.array_equal(index[index], np.arange(C)) and np.all(sign * sign[index] == 1.0) and set(np.unique(sign)) <= {-1.0, 1.0}, group
        assert (index != np.arange(C)).any() or C <= 2, group            # a mirror, not the identity
    mt = mirror_tables(skel)
    assert np.array_equal(maps["actions"][0], mt.dof_perm) and np.array_equal(maps["actions"][1], mt.dof_sign)


# ---- 2. refusals by name ---------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_key_or_body():
    name = "v2_g1_29dof_teacher.yaml"

    def relyaw(cfg):
        cfg.obs.obs_dict["actor_obs"] = list(cfg.obs.obs_dict["actor_obs"]) + ["relyaw"]
        cfg.obs.obs_scales["relyaw"], cfg.obs.noise_scales["relyaw"] = 1.0, 0.0
        cfg.obs.obs_dims.append({"relyaw": 1})

    cfg, skel, _, _ = _cpu_build(name, mutate=relyaw)
    with pytest.raises((_lib.PbhcError, NotImplementedError), match=r"'relyaw' has no mirror rule"):
        obs_mirror.build(cfg, skel)

    def one_knee(cfg):
        cfg.robot.key_bodies = [b for b in cfg.robot.key_bodies if b != "left_knee_link"]
        cfg.robot.num_key_bodies = len(cfg.robot.key_bodies)

    cfg, skel, _, _ = _cpu_build(name)
    one_knee(cfg)
    with pytest.raises((_lib.PbhcError, NotImplementedError), match=r"robot\.key_bodies lists 'right_knee_link' without its partner 'left_knee_link'"):
        obs_mirror.build(cfg, skel)

    cfg, skel, _, _ = _cpu_build(name)
    cfg.robot.motion["anchor_link"] = "pelvis"
    with pytest.raises((_lib.PbhcError, NotImplementedError), match=r"anchor_link 'pelvis' resolves to body 'left_hip_pitch_link'"):
        obs_mirror.build(cfg, skel)
    cfg.robot.motion["anchor_link"] = "pelvis_link"                       # the default: body 0 through the reference's `+ 1`
    obs_mirror.build(cfg, skel)

    cfg, skel, _, _ = _cpu_build(name)
    cfg.robot.init_state.default_joint_angles["left_knee_joint"] = 0.35
    with pytest.raises((_lib.PbhcError, NotImplementedError), match=r"default_joint_angles of '(left|right)_knee_joint'"):
        obs_mirror.build(cfg, skel)

    cfg, skel, _, _ = _cpu_build(name)
    cfg.domain_rand.randomize_link_body_names = [b for b in cfg.domain_rand.randomize_link_body_names if b != "right_elbow_link"]
    with pytest.raises((_lib.PbhcError, NotImplementedError), match=r"randomize_link_body_names lists 'left_elbow_link' without its partner"):
        obs_mirror.build(cfg, skel)


# ---- 3. equivariance against the oracle --------------------------------------------------------------------------------------------------
CASES = {"student23": ("v2_g1_23dof_student.yaml", "g1_23dof", "g1_ue_walk_23dof.npz", 96.0 / 30.0),
         "teacher29": ("v2_g1_29dof_teacher.yaml", "g1_29dof", CLIP29, 397.0 / 30.0)}
STEPS = 12
POLAR, AXIAL, QUAT = np.array([1.0, -1.0, 1.0], np.float32), np.array([-1.0, 1.0, -1.0], np.float32), np.array([-1.0, 1.0, -1.0, 1.0], np.float32)
# the reference quantities an element of a reference-derived observation key depends on (one step of it); every other key with a rule reads
# the robot's own state, the DR draws or the actions, which the test mirrors exactly
REF_TOL = {
    "future_motion_root_height": ["root_pos"], "future_motion_roll_pitch": ["root_rot"], "future_motion_base_lin_vel": ["root_vel", "root_rot"],
    "future_motion_base_ang_vel": ["root_ang_vel", "root_rot"], "future_motion_base_yaw_vel": ["root_ang_vel", "root_rot"],
    "future_motion_dof_pos": ["dof_pos"], "future_motion_local_ref_key_body_pos": ["body_pos", "root_rot"],
    "anchor_ref_pos": ["root_pos"], "anchor_ref_rot": ["root_rot"], "ref_motion_phase": [],
    "dif_root_height": ["root_pos"], "dif_root_velocity": ["root_vel", "root_rot"], "dif_root_rot": ["root_rot"],
    "dif_joint_angles": ["dof_pos"], "dif_joint_velocities": ["dof_vel"], "ref_contact_mask": [],
}
ROBOT_FK_KEYS = {"local_key_body_pos"}                                    # positions out of the robot's own forward kinematics
DELTA_CAPS = {"root_pos": 1e-6, "root_rot": 1e-6, "root_vel": 1e-4, "root_ang_vel": 1e-4, "dof_pos": 0.0, "dof_vel": 0.0}


class Mirrored:
    """The construction of the module docstring for one config: the two-clip oracle library, the inputs of 2n envs (`src` / `mir`: the env
    indices of the two halves, pairwise), the per-element bounds."""

    def __init__(self, tag, n=4, src=None, mir=None, seed=11):
        from oracle.env_v2 import GeneralTrackingOracle
        from oracle.motion_lib import MotionLib as OML

        cfgname, robot, clipname, self.start = CASES[tag]
        self.tag, self.n, N = tag, n, 2 * n
        self.src = np.arange(n) if src is None else np.asarray(src)
        self.mir = np.arange(n, N) if mir is None else np.asarray(mir)
        self.cfg = cfg = fixture_config(cfgname, N, {"domain_rand.push_robots": False})
        self.sk, self.osk = skeleton(robot), skel_from_golden(robot)
        self.mt = mt = mirror_tables(self.sk, 1e-4)
        self.maps = obs_mirror.build(cfg, self.sk)
        clip = load_clip(clipname)
        pose, trans, contact = restate(clip, True, 1.0, mt.body_perm)
        mclip = dict(clip, pose_aa=pose, root_trans_offset=trans)
        if contact is not None:
            mclip["contact_mask"] = contact
        self.clips = [clip, mclip]
        self.oml = OML(self.osk, self.clips)
        self.D, self.B = D, B = self.sk.num_dof, self.sk.num_bodies
        g = torch.Generator().manual_seed(seed)
        half = lambda x: self.both(x, None)
        # ---- DR the simulator owns, and the episodic draws: the second half the mirror of the first
        nl = len(cfg.domain_rand.randomize_link_body_names)
        link_perm = obs_mirror._list_perm(cfg.domain_rand.randomize_link_body_names, "links")
        com = (torch.rand(n, 3, generator=g) - 0.5) * 0.1
        mass = 0.9 + 0.2 * torch.rand(n, nl, generator=g)
        fric = 0.2 + torch.rand(n, 1, 1, generator=g)
        base_mass = 0.9 + 0.2 * torch.rand(n, 1, generator=g)
        self.dr = dict(base_com_bias=self.both(com, com * torch.from_numpy(POLAR)), link_mass_scale=self.both(mass, mass[:, link_perm]),
                       friction_coeffs=self.both(fric, fric), base_mass_scale=self.both(base_mass, base_mass))
        self.orc = orc = GeneralTrackingOracle(cfg, self.osk, self.oml, N, self.dr)
        orc.slot_clip = torch.zeros(N, dtype=torch.long)
        orc.slot_clip[self.mir] = 1
        orc.motion_ids = orc.slot_clip.clone()
        self.dt = orc.dt
        start = torch.full((N,), self.start)
        st = {k: v.clone() for k, v in orc.s.items()}
        st["motion_start_times"], st["motion_len"] = start, self.oml.motion_len[orc.slot_clip].clone()
        st["reset_buf"] = torch.zeros(N, dtype=torch.long)
        perm, sign = torch.from_numpy(mt.dof_perm), torch.from_numpy(mt.dof_sign)
        self.dof = lambda x: x[..., perm] * sign
        unsigned = lambda x: x[..., perm]
        for name, lo, w, m in (("kp_scale", 0.9, 0.2, unsigned), ("kd_scale", 0.9, 0.2, unsigned), ("rfi_lim_scale", 0.5, 1.0, unsigned), ("rao_scale", -0.05, 0.1, self.dof)):
            x = lo + w * torch.rand(n, D, generator=g)
            st[name] = self.both(x, m(x))
        delay = torch.randint(0, 3, (n,), generator=g)
        st["action_delay_idx"] = self.both(delay, delay)
        self.samp = {k: st[k].clone() for k in ("motion_start_times", "kp_scale", "kd_scale", "rfi_lim_scale", "rao_scale", "action_delay_idx")}
        # ---- replay frames: the source's reference + a perturbation, and its mirror image
        from tests.helpers import synth_replay

        T = STEPS + 1
        root, qp, qv, cf = synth_replay(self.oml, self.osk, n, T, torch.full((n,), self.start), torch.zeros(n, dtype=torch.long), self.dt, torch.zeros(n, 3), seed + 1, orc.feet)
        body_perm = torch.from_numpy(mt.body_perm[:B])
        assert int(body_perm.max()) < B
        mroot = torch.cat([root[..., 0:3] * torch.from_numpy(POLAR), root[..., 3:7] * torch.from_numpy(QUAT), root[..., 7:10] * torch.from_numpy(POLAR),
                           root[..., 10:13] * torch.from_numpy(AXIAL)], dim=-1)
        self.root, self.qp, self.qv = self.both(root, mroot, 1), self.both(qp, self.dof(qp), 1), self.both(qv, self.dof(qv), 1)
        self.cf = self.both(cf, cf[:, :, body_perm] * torch.from_numpy(POLAR), 1)
        st["root_states"], st["dof_pos"], st["dof_vel"], st["contact_forces"] = self.root[0], self.qp[0], self.qv[0], self.cf[0]
        self.flat = {k: v.numpy() for k, v in st.items()}
        for k in orc.sums:
            self.flat["sum__" + k] = np.zeros(N, np.float32)
        for k in orc.hist:
            self.flat["hist__" + k] = np.zeros(tuple(orc.hist[k].shape), np.float32)
        for k in orc.sigma:
            self.flat["sigma__" + k] = orc.sigma[k]
        self.flat.update(reward_penalty_scale=1.0, average_episode_length=0.0, motion_far_threshold=1.5)
        act = 0.5 * torch.randn(STEPS, n, D, generator=g)
        u = torch.rand(STEPS, n, D, generator=g)
        self.act, self.u = self.both(act, self.dof(act), 1), self.both(u, 0.5 + (u[..., perm] - 0.5) * sign, 1)
        self._bounds()

    def both(self, a, b, dim=0):
        """a tensor over all 2n envs (axis `dim`) from the first half's `a` and the second half's `b`"""
        shape = list(a.shape)
        shape[dim] = 2 * self.n
        out = torch.zeros(shape, dtype=a.dtype)
        out.index_copy_(dim, torch.from_numpy(self.src), a)
        out.index_copy_(dim, torch.from_numpy(self.mir), a if b is None else b)
        return out

    def frame(self, k):
        return dict(root=self.root[k + 1], dof_pos=self.qp[k + 1], dof_vel=self.qv[k + 1], contact=self.cf[k + 1])

    def _bounds(self):
        """delta_q over every time the test reads, the precondition on the angular velocity, and the per-element tolerance of every group"""
        cfg, mt, oml = self.cfg, self.mt, self.oml
        steps = np.arange(0, STEPS + 1 + int(cfg.obs.future_max_steps) + 1)
        t = torch.tensor(self.start + steps * self.dt, dtype=torch.float32)
        a = oml.get_motion_state(torch.zeros(len(t), dtype=torch.long), t)
        b = oml.get_motion_state(torch.ones(len(t), dtype=torch.long), t)
        perm = torch.from_numpy(mt.body_perm)
        dmax = lambda x, y: float((x.double() - y.double()).abs().max())
        qa = a["root_rot"] * torch.from_numpy(QUAT)
        self.delta = d = {
            "root_pos": dmax(b["root_pos"], a["root_pos"] * torch.from_numpy(POLAR)), "root_vel": dmax(b["root_vel"], a["root_vel"] * torch.from_numpy(POLAR)),
            "root_ang_vel": dmax(b["root_ang_vel"], a["root_ang_vel"] * torch.from_numpy(AXIAL)),
            "root_rot": float(torch.minimum((b["root_rot"] - qa).abs().amax(-1), (b["root_rot"] + qa).abs().amax(-1)).max()),
            "dof_pos": dmax(b["dof_pos"], self.dof(a["dof_pos"])), "dof_vel": dmax(b["dof_vel"], self.dof(a["dof_vel"])),
            "body_pos": dmax(b["rg_pos_t"], a["rg_pos_t"][:, perm] * torch.from_numpy(POLAR)),
        }
        depth = int(self.sk.depth.max())
        self.fk_tol = (depth + 2) * mt.asymmetry
        print(f"{self.tag}: " + ", ".join(f"delta {k} {v:.3e}" for k, v in d.items()) + f"; robot FK (depth {depth} + 2) x a {mt.asymmetry:.3e} = {self.fk_tol:.3e}")
        assert d["root_ang_vel"] <= 1e-4, "precondition: the two libraries' root angular velocities are mirror images at every time read"
        for k, cap in DELTA_CAPS.items():
            assert d[k] <= cap, (k, d[k], cap)
        assert d["body_pos"] <= self.fk_tol
        bld = obs_mirror._Builder(cfg, self.sk, 1e-4)

        def key_delta(k):
            """per element of ONE step of key k: the deltas of what it depends on"""
            if k == "next_step_ref_motion":
                return np.concatenate([key_delta(p) for p in obs_mirror.NEXT_STEP_PARTS])
            extra = sum(d[q] for q in REF_TOL.get(k, [])) + (self.fk_tol if k in ROBOT_FK_KEYS else 0.0)
            return np.full(len(bld.step_map(k)[0]), extra)

        self.tol = {}
        for group, keys in cfg.obs.obs_dict.items():
            parts = []
            for key in sorted(keys):
                k = obs_mirror.rule_key(key)
                width = len(bld.key_map(key)[0])
                if k in cfg.obs.obs_auxiliary:                               # history: the robot's own state and the actions
                    parts.append(np.zeros(width))
                    continue
                one = key_delta(k)
                parts.append(abs(float(cfg.obs.obs_scales[k])) * np.tile(one, width // len(one)))
            self.tol[group] = np.concatenate(parts)
            assert len(self.tol[group]) == len(self.maps[group][0])

    def check(self, obs, what, mirrored_first_half=None):
        """obs {group: [2n, C] array}: the second half against the map applied to the first (or against `mirrored_first_half`, the same thing
        computed by the code under test), element by element"""
        for group, x in obs.items():
            x = np.asarray(x, np.float64)
            want = obs_mirror.apply(self.maps[group], x[self.src]) if mirrored_first_half is None else np.asarray(mirrored_first_half[group], np.float64)
            got = x[self.mir]
            bound = self.tol[group][None, :] + 3e-5 + 3e-5 * np.abs(want)
            err = np.abs(got - want)
            j = np.unravel_index(np.argmax(err - bound), err.shape)
            assert np.all(err <= bound), f"{what} {group}: element {j[1]} of env pair {j[0]}: {got[j]:.6g} vs mirrored {want[j]:.6g}, |err| {err[j]:.3e} > {bound[j]:.3e}"


@pytest.mark.parametrize("tag", sorted(CASES))
def test_oracle_observations_are_equivariant_under_the_maps(tag):
    from oracle.fk import sim_fk

    m = Mirrored(tag)
    orc = m.orc
    orc.load_state(m.flat)
    nonzero = {g: np.zeros(len(m.maps[g][0]), bool) for g in m.cfg.obs.obs_dict}
    for k in range(STEPS):
        fr = m.frame(k)
        obs, _, reset, _ = orc.step(m.act[k], fr, sim_fk(m.osk, fr["root"], fr["dof_pos"], fr["dof_vel"]), u_rfi=m.u[k], reset_samples=m.samp)
        assert int(reset.sum()) == 0, "an env was reset: the perturbation is too large for this test"
        m.check({g: v.numpy() for g, v in obs.items()}, f"{tag} step {k}")
        for g, v in obs.items():
            nonzero[g] |= (v.numpy()[m.src] != 0.0).any(0)
    # no element is left out, and none passes by being zero throughout (masked joint velocities are zero by definition)
    for g, nz in nonzero.items():
        dead = np.nonzero(~nz)[0]
        assert len(dead) <= (4 * (1 + m.cfg.obs.history_length) if m.cfg.obs.get("masked_dof_vel", False) else 0), (g, dead[:20])
    # and a wrong sign is not within the bounds: the identity map fails
    ident = copy.copy(m)
    ident.maps = {g: (np.arange(len(i), dtype=np.int32), np.ones(len(i), np.float32)) for g, (i, s) in m.maps.items()}
    with pytest.raises(AssertionError):
        ident.check({g: v.numpy() for g, v in obs.items()}, "identity")
