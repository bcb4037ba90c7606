"""CPU: the launch plan of k_fixed_msm (csrc/fixed_plan.hpp) as a host build (g++) of the header the kernel and the
verifier's host side compile (tests/host/fixed_plan_host_test.cpp): blocks per proof against the formula the plan was added
to, where long blocks engage, and the map from a block of the grid to (proof, part) -- which decides the scalars and table
rows a block gathers -- as a bijection at every swept launch."""

import os
import subprocess

import pytest

import mulvec_cases as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("BPP_HOST_SANITIZE") else []
RES = 1024
NFS = (10, 66, 130, 258, 514, 1026, 2050, 8194)
COUNTS = 4200 + 3


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fixed_plan") / ("bpp_fixed_plan_host_test" + ("_san" if SANITIZE else "")))
    subprocess.check_call(["g++", "-O2", "-std=c++17"] + SANITIZE + ["-o", out, os.path.join(ROOT, "tests", "host", "fixed_plan_host_test.cpp")])
    return out


def _plans(exe, cases):
    out = subprocess.check_output([exe, "plan"] + ["%d:%d:%d" % t for t in cases]).decode().splitlines()
    assert len(out) == len(cases)
    return [tuple(int(x) for x in line.split()) for line in out]


def test_sweep_per_rule_bijection_and_block_count(exe):
    out = subprocess.check_output([exe, "sweep"]).decode().split()
    assert out[0] == "ok" and int(out[2]) == len(NFS) * COUNTS * 4
    # planned: form 0, NF in {1026, 2050, 8194}, every count above RES but 40000 (per is 1 there)
    assert int(out[3]) == 3 * (4200 - RES + 2)


def test_every_existing_gpu_case_is_launched_as_before(exe):
    """the cases of GPU_CASES pin the hook's geometry to [form, blocks]: no plan may engage at any of them"""
    cases = []
    for cname, n, m, c, count, mv, form, blocks in M.GPU_CASES:
        cases.append((M.Shape(cname, n, mv or m, c).NF, count, form))
    assert max(nf for nf, _, _ in cases) <= 514
    for (nf, count, form), (per, longs, nblk), case in zip(cases, _plans(exe, cases), M.GPU_CASES):
        assert (per, longs, nblk) == (case[7], 0, count * case[7]), case
    # ... nor at these shapes in any other form or at any count up to the largest the tests use
    more = [(nf, count, form) for nf in (10, 66, 130, 258, 514) for count in (1, 205, 1024, 1025, 1100, 2100, 8192) for form in range(4)]
    assert all(longs == 0 and nblk == count * per for (_, count, _), (per, longs, nblk) in zip(more, _plans(exe, more)))


def test_the_shapes_where_the_plan_engages(exe):
    """the headline pass (n=64, m=16, 8192 proofs) and the shapes of tests/test_gpu_fixed_plan.py"""
    got = _plans(exe, [(2050, 8192, 0), (2050, 1100, 0), (1026, 1024, 0), (1026, 1025, 0), (1026, 1100, 0), (1026, 2100, 0),
                       (1026, 1100, 2), (2050, 40000, 0), (2050, 550, 0), (2050, 3200, 0)])
    assert got == [(4, 7168, 7168 + 1024 * 4), (4, 76, 76 + 1024 * 4), (2, 0, 2048), (2, 1, 1 + 2048), (2, 76, 76 + 2048),
                   (2, 1076, 1076 + 2048), (2, 0, 2200), (1, 0, 40000), (4, 0, 2200), (4, 2176, 2176 + 1024 * 4)]
    # 32 768 blocks of partials become 11 264
    assert got[0][2] == 11264


def test_block_map_at_the_zone_boundary(exe):
    out = subprocess.check_output([exe, "map", "4", "7168", "0", "7167", "7168", "7171", "7172", "11263"]).decode().splitlines()
    assert [tuple(int(x) for x in line.split()) for line in out] == [
        (0, 0, 1), (7167, 0, 1), (7168, 0, 4), (7168, 3, 4), (7169, 0, 4), (8191, 3, 4)]
    out = subprocess.check_output([exe, "map", "3", "0", "0", "2", "3", "7"]).decode().splitlines()
    assert [tuple(int(x) for x in line.split()) for line in out] == [(0, 0, 3), (0, 2, 3), (1, 0, 3), (2, 1, 3)]
