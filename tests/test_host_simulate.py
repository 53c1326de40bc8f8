"""CPU tests of the simulation feature: the NumPy Philox4x32-10 restatement the GPU tests compare against, and the command line of
vidp_amd.generate_data."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import np_sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr, key, expect", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
], ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, expect):
    """The published Philox4x32-10 known-answer vectors (Random123's kat_vectors)."""
    out = np_sim.philox4x32_10(ctr, key)
    assert [int(w) for w in out] == list(expect)


def test_uniforms_are_in_the_open_unit_interval_from_below():
    assert np_sim.uniform53(0, 0) == 0.5 * 2.0 ** -53
    assert np_sim.uniform53(0xffffffff, 0xffffffff) <= 1.0
    assert np_sim.uniform53(0x800, 0) == 1.5 * 2.0 ** -53


def test_normal_restatement_shapes_and_odd_dimension():
    z3 = np_sim.normals(5, 0, [0, 7], [0, 1, 2], 3)
    z4 = np_sim.normals(5, 0, [0, 7], [0, 1, 2], 4)
    assert z3.shape == (2, 3, 3)
    np.testing.assert_array_equal(z3, z4[..., :3])       # odd d drops the last sine
    assert not np.array_equal(z3, np_sim.normals(6, 0, [0, 7], [0, 1, 2], 3))


def test_generate_data_command_line_parses():
    from vidp_amd import generate_data as g
    a = g.parse_args(["-sde", "ou", "-d", "0.7", "-q", "0.8", "-t0", "0", "-t1", "2", "-x0", "0.5", "-dt", "0.01", "-n", "30", "-si", "0.2",
                      "-o", "out", "-s", "4", "-dim", "2"])
    assert (a.sde, a.decay, a.diffusion, a.t0, a.t1, a.x0, a.dt, a.num_observations, a.sigma, a.output, a.seed, a.dim) == \
        ("ou", 0.7, 0.8, 0.0, 2.0, 0.5, 0.01, 30, 0.2, "out", 4, 2)
    a = g.parse_args(["-sde", "vanderpol", "-dim", "2"])
    assert (a.t1, a.dt, a.num_observations, a.seed) == (1.0, 0.01, 10, 33)
    tg = g.time_grid_of(0.0, 1.0, 0.01)
    assert tg.shape == (101,) and tg[0] == 0.0 and tg[-1] == 1.0 and np.all(np.diff(tg) > 0)


@pytest.mark.parametrize("argv, msg", [
    (["-sde", "brownian"], "invalid choice"),
    ([], "required"),
    (["-sde", "ou", "-dt", "0"], "-dt must be positive"),
    (["-sde", "ou", "-t0", "2", "-t1", "1"], "t0 <= t1"),
    (["-sde", "ou", "-n", "500"], "-n must be between"),
    (["-sde", "vanderpol"], "two state dimensions"),
    (["-sde", "ou", "-dim", "0"], "-dim must be at least 1"),
    (["-sde", "ou", "-n", "many"], "invalid int value"),
])
def test_generate_data_argument_errors(argv, msg, capsys):
    from vidp_amd import generate_data as g
    with pytest.raises(SystemExit) as e:
        g.parse_args(argv)
    assert e.value.code == 2
    assert msg in capsys.readouterr().err


def test_generate_data_runs_as_a_module():
    """`python -m vidp_amd.generate_data` from the repository root: --help and an argument error, no GPU touched."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "vidp_amd.generate_data", "--help"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "-sde" in r.stdout
    r = subprocess.run([sys.executable, "-m", "vidp_amd.generate_data", "-sde", "ou", "-dt", "-1"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 2 and "-dt must be positive" in r.stderr
