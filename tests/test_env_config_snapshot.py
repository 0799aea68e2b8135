"""Everything env_config.build produces — every member of PbhcEnvConfig, the observation maps, the compact map image, the initial globals
and the rest of the EnvLayout — against tests/golden/env_config_snapshot.json, per case of tools/gen_env_config_snapshot.py: the five
fixture trees plain and with the switches the other tests and the reference traces exercise.  The config-specialised step kernel is
compiled from the text of that struct and cached under a hash of it, so a member that moves silently is a different kernel; a failure names
the members that moved.  No GPU, no compiled library (`build` with device "cpu" needs the header only)."""
import json

import pytest

from tools.gen_env_config_snapshot import CASES, FIXTURE, build_case, snapshot

SNAPSHOT = json.load(open(FIXTURE))


def test_fixture_holds_exactly_the_cases():
    assert sorted(SNAPSHOT) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_build_output_is_the_recorded_one(monkeypatch, name):
    from pbhc_amd.envs import env_config

    case = CASES[name]
    monkeypatch.delenv("PBHC_ROW_HELP_SHARE", raising=False)
    monkeypatch.delenv("PBHC_ROLE0_HANDICAP", raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setattr(env_config, "PACKED_MAPS", case["packed"])
    c, L = build_case(case)
    got, want = snapshot(c, L), SNAPSHOT[name]
    for part in ("config", "layout"):
        moved = sorted(k for k in set(got[part]) | set(want[part]) if got[part].get(k) != want[part].get(k))
        assert not moved, f"{name}: {part} members that differ from the snapshot: {moved}"
    if name.startswith("row_help_share/"):
        assert L.helper_elements > 100                      # (the share really hands runs to the dynamics waves: tests/test_gpu_specialise.py)
    if name.startswith("maps_not_packed/"):
        assert L.map_image is None and c.map_lds_words == 0
