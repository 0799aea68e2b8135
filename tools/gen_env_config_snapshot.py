"""Snapshot of everything `pbhc_amd/envs/env_config.build` produces, for tests/test_env_config_snapshot.py (CPU, no compiled library).

tests/golden/env_config_snapshot.json holds, per case of CASES, one short digest per top-level member of PbhcEnvConfig (over a canonical
text of its value: recursing into `skel` and every `groups[i]` with its `runs`, floats as their exact hex, a pointer only as null / nonnull)
and one per EnvLayout attribute (tensors and arrays over dtype, shape and bytes; everything else over its JSON).  An attribute that is
absent counts as its declared default (`future_steps` [], `map_image` None).  The config-specialised step kernel is compiled from the text
of that struct, so a digest that moves is a different kernel: regenerate this file only when a feature is MEANT to change the layout, and
review which members moved —

    PYTHONPATH=<repo> python tools/gen_env_config_snapshot.py            writes the fixture
    PYTHONPATH=<repo> python tools/gen_env_config_snapshot.py --check    builds every case again (a fresh process) and compares
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys
from unittest import mock

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests.helpers import GOLDEN, SOFT_LIMIT_OVERRIDES, TERM_NOISE_OVERRIDES, build_env_config      # noqa: E402
from tests.test_imu_noise_dr_cpu import OU, PS_PD, PS_TAU, add_noise_names                          # noqa: E402
from tests.test_oracle_env import SWITCH_CASES                                                      # noqa: E402
from tests.test_record_cpu import RECORD                                                            # noqa: E402
from tests.test_reset_options_cpu import DOF_FAR, NOISE                                             # noqa: E402
from tools.gen_obs_reward_terms_golden import overrides as terms_overrides                          # noqa: E402

FIXTURE = os.path.join(GOLDEN, "env_config_snapshot.json")
HORSE, WALK = "v1_g1_23dof_horse_stance.yaml", "v1_g1_23dof_walk.yaml"
STUDENT, TEACHER, TEACHER29 = "v2_g1_23dof_student.yaml", "v2_g1_23dof_teacher.yaml", "v2_g1_29dof_teacher.yaml"
_T, _TS = "env.config.termination.", "env.config.termination_scales."
# tests/test_gpu_parity.py: test_env_step_close_to_limit_terminations / test_env_step_randomized_default_dof_pos_matches_oracle
CLOSE_TO_LIMITS = {_T + "terminate_when_close_to_dof_pos_limit": True, _T + "terminate_when_close_to_dof_vel_limit": True,
                   _T + "terminate_when_close_to_torque_limit": True, _TS + "termination_close_to_dof_pos_limit": 0.55,
                   _TS + "termination_close_to_dof_vel_limit": 0.02, _TS + "termination_close_to_torque_limit": 0.35}
DEFAULT_DOF_POS = {"domain_rand.randomize_default_dof_pos": True, "domain_rand.dof_pos_range": [-0.05, 0.05]}


def _terms(cfgname):
    from pbhc_amd.utils.config import load_config

    return terms_overrides(load_config(os.path.join(GOLDEN, "configs", cfgname), {"num_envs": 8}, now="t"), cfgname.startswith("v2_"))


def _case(cfgname, overrides=None, mutate=None, env=None, packed=True):
    return dict(cfgname=cfgname, overrides=overrides or {}, mutate=mutate, env=env or {}, packed=packed)


# name -> the tree, its overrides and the switches outside the tree (environment variables; env_config.PACKED_MAPS, read at import)
CASES = {"plain/" + n[:-5]: _case(n) for n in (HORSE, WALK, STUDENT, TEACHER, TEACHER29)}
CASES.update({
    "ou_ps_noise_names/walk": _case(WALK, dict(OU, **PS_PD, **PS_TAU), add_noise_names),
    "ou_ps_noise_names/student": _case(STUDENT, dict(OU, **PS_PD, **PS_TAU), add_noise_names),
    "dof_far_reset_noise/walk": _case(WALK, dict(DOF_FAR, **NOISE)),
    "reset_noise/student": _case(STUDENT, NOISE),
    "terms/walk": _case(WALK, lambda: _terms(WALK)),
    "terms/student": _case(STUDENT, lambda: _terms(STUDENT)),
    "save_motion/walk": _case(WALK, RECORD),
    "soft_limit_curriculum/walk": _case(WALK, SOFT_LIMIT_OVERRIDES),
    "term_contact_height_noise_curriculum/walk": _case(WALK, TERM_NOISE_OVERRIDES),
    "close_to_limits/walk": _case(WALK, CLOSE_TO_LIMITS),
    "default_dof_pos/walk": _case(WALK, DEFAULT_DOF_POS),
    "masked_dof_vel/student": _case(STUDENT, {"obs.masked_dof_vel": True}),
    "maps_not_packed/horse_stance": _case(HORSE, packed=False),
    "maps_not_packed/teacher": _case(TEACHER, packed=False),
    # tests/test_gpu_specialise.py runs this share (on the walk tree); horse_stance resolves the same way: every row with role 1
    "row_help_share/horse_stance": _case(HORSE, env={"PBHC_ROW_HELP_SHARE": "0.23"}),
    "role0_handicap/student": _case(STUDENT, env={"PBHC_ROLE0_HANDICAP": "1.0"}),
})
CASES.update({"switch/" + tag: _case(cfgname, ov) for tag, cfgname, ov in SWITCH_CASES[:3]})        # control types V / T, the foot-orientation terms


def build_case(case):
    """(c, L) of a case; the caller has applied case['env'] and case['packed'] (switches: the generator's own, monkeypatch in the test)"""
    ov = case["overrides"]
    general = case["cfgname"].startswith("v2_")
    return build_env_config(case["cfgname"], ov() if callable(ov) else ov, num_envs=8, seed=0, general=general,
                            has_contact_mask="walk" not in case["cfgname"], mutate=case["mutate"])[2:]


@contextlib.contextmanager
def switches(case):
    from pbhc_amd.envs import env_config

    with mock.patch.dict(os.environ, case["env"]), mock.patch.object(env_config, "PACKED_MAPS", case["packed"]):
        yield


def _text(v, ct):
    """canonical text of a ctypes value of type `ct`"""
    if issubclass(ct, C.Structure):
        return "{" + ";".join(f"{name}={_text(getattr(v, name), ft)}" for name, ft in ct._fields_) + "}"
    if issubclass(ct, C.Array):
        return "[" + ",".join(_text(v[i], ct._type_) for i in range(ct._length_)) + "]"
    if ct is C.c_void_p:
        return "null" if not v else "nonnull"
    return float(v).hex() if isinstance(v, float) else str(int(v))


def _sha(data):
    return hashlib.sha256(data if isinstance(data, bytes) else data.encode()).hexdigest()[:12]


def _array(a):
    a = np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a)
    return _sha(f"{a.dtype}{a.shape}".encode() + a.tobytes())


def _plain(v):
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return v.item() if isinstance(v, np.generic) else v


def snapshot(c, L):
    """{"config": {member: digest}, "layout": {attribute: digest}}"""
    attrs = dict(vars(L))
    attrs.setdefault("future_steps", [])
    attrs.setdefault("map_image", None)
    layout = {}
    for k, v in sorted(attrs.items()):
        if k == "map_tensors":
            for i, quad in enumerate(v):
                for name, t in zip(("dst", "src", "scale", "noise"), quad):
                    layout[f"map_tensors[{i}].{name}"] = _array(t)
        elif isinstance(v, (torch.Tensor, np.ndarray)):
            layout[k] = _array(v)
        else:
            layout[k] = _sha(json.dumps(_plain(v)))               # (dict order kept: it is the order the env iterates in)
    return {"config": {name: _sha(_text(getattr(c, name), ft)) for name, ft in type(c)._fields_}, "layout": layout}


def record():
    out = {}
    for name, case in CASES.items():
        with switches(case):
            out[name] = snapshot(*build_case(case))
    return out


def check_recording(snap):
    """what the cases are there for: the switch variants really resolve to something other than the plain build"""
    plain = lambda n: snap["plain/" + n]
    assert snap["row_help_share/horse_stance"]["layout"]["helper_elements"] != plain("v1_g1_23dof_horse_stance")["layout"]["helper_elements"]
    assert snap["role0_handicap/student"]["layout"]["group_roles"] != plain("v2_g1_23dof_student")["layout"]["group_roles"]
    for n in ("horse_stance", "teacher"):
        assert snap["maps_not_packed/" + n]["layout"]["map_image"] == _sha(json.dumps(None))


if __name__ == "__main__":
    snap = record()
    check_recording(snap)
    if "--check" in sys.argv:
        want = json.load(open(FIXTURE))
        moved = [f"{case}: {part}.{k}" for case in want for part in want[case] for k in want[case][part] if snap.get(case, {}).get(part, {}).get(k) != want[case][part][k]]
        moved += [f"{case}: not in the fixture" for case in snap if case not in want]
        print("\n".join(moved) or f"{len(snap)} cases agree with {os.path.relpath(FIXTURE, ROOT)}")
        sys.exit(1 if moved else 0)
    with open(FIXTURE, "w") as f:
        json.dump(snap, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(snap)} cases -> {os.path.relpath(FIXTURE, ROOT)} ({os.path.getsize(FIXTURE)} bytes)")
