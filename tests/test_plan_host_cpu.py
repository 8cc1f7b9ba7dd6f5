"""The collective planner without a GPU: tools/plan_host_check.c, compiled by
gcc around libfabric_amd/csrc/lfa_coll_plan.c, plans and lowers a grid of
collectives and prints one digest line per (collective, algorithm, group size).
The lines are compared with tests/golden/plan_digests.txt (and _knobs.txt, the
run with the one-shot bounds overridden), which were recorded from the planner
as it was before its rewrite: every schedule stays bit for bit what it was.
The program is built once more with ASan + UBSan and run stand-alone over the
core cases of each line (--core), whose digest the recorded lines carry beside
the one over the whole grid."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "plan_host_check.c")
GOLDEN = os.path.join(ROOT, "tests", "golden")
KNOBS = ("65536", "131072")        # LFA_OS_AG_BYTES, LFA_OS_RS_BYTES
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _build(tmp_path, name, *flags):
    exe = str(tmp_path / name)
    r = subprocess.run(["gcc", "-std=gnu11", "-O2", "-g", "-Wall", "-Wextra", "-Werror", *flags,
                        "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "libfabric_amd", "csrc"),
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return f.read().splitlines()


SIZES = {1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 31, 32, 33, 47, 48, 64, 100, 511, 512, 513, 1100}
COLLS = {"barrier", "broadcast", "alltoall", "allreduce", "allgather", "reduce_scatter", "reduce",
         "scatter", "gather"}
ALGOS = {"tree", "rd", "rccl", "tree_coll", "p2p", "auto"}


def _compare(got, want, core_only):
    """Line by line, so that a mismatch names the collective, algorithm and n.
    A --core run leaves the full digest out: its lines are compared up to it."""
    got = got.splitlines()
    for g, w in zip(got, want):
        if core_only and not w.startswith("#"):
            assert g.endswith(" full=-")
            g, w = g.split()[:-1], w.split()[:-1]
        assert g == w
    assert len(got) == len(want)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The plain build over the whole grid and the sanitizer build over the
    core cases, each without and with the knobs, side by side."""
    tmp = tmp_path_factory.mktemp("plan")
    cmds = {"plain": [_build(tmp, "plan_host_check")],
            "san": [_build(tmp, "plan_host_check_san", *SANITIZE), "--core"]}
    procs = {(kind, knobs): subprocess.Popen([*cmd, *knobs], stdout=subprocess.PIPE,
                                             stderr=subprocess.PIPE, text=True)
             for kind, cmd in cmds.items() for knobs in ((), KNOBS)}
    out = {}
    for key, p in procs.items():
        stdout, stderr = p.communicate()
        out[key] = (p.returncode, stdout, stderr)
    return out


@pytest.mark.parametrize("kind", ["plain", "san"])
@pytest.mark.parametrize("knobs,golden", [((), "plan_digests.txt"),
                                          (KNOBS, "plan_digests_knobs.txt")])
def test_plans_match_the_recorded_digests(runs, kind, knobs, golden):
    rc, stdout, stderr = runs[(kind, knobs)]
    assert rc == 0, stderr
    _compare(stdout, _golden(golden), core_only=kind == "san")


def test_the_program_walks_every_collective_algorithm_and_size(runs):
    rc, stdout, stderr = runs[("plain", ())]
    assert rc == 0, stderr
    lines = [ln.split() for ln in stdout.splitlines() if not ln.startswith("#")]
    assert {ln[0] for ln in lines} == COLLS
    assert {ln[1] for ln in lines} == ALGOS
    assert {int(ln[2][2:]) for ln in lines} == SIZES
    assert len(lines) == len(COLLS) * len(ALGOS) * len(SIZES)
    for ln in lines:
        n = int(ln[2][2:])
        core, full = (int(f.split("=")[1].split(":")[0].split("/")[1]) for f in ln[4:6])
        # every rank up to 64 (five above), both roots, three element sizes and
        # at least the nine fixed counts less the ones that coincide (n <= 8)
        ranks, roots = (n if n <= 64 else 3), (2 if n > 1 else 1)
        assert full >= 4 + ranks * roots * 3 * 6 and core <= full, ln
        assert (core == full) == (n <= 9), ln
    # RCCL is not a schedule: its plans are TREE's
    tree = {(ln[0], ln[2]): ln[3:] for ln in lines if ln[1] == "tree"}
    assert all(ln[3:] == tree[(ln[0], ln[2])] for ln in lines if ln[1] == "rccl")
    # what is not planned answers -LFA_ENOSYS (38)
    assert all(ln[3] == "rc=-38" for ln in lines
               if ln[1] == "auto" or ln[0] in ("barrier", "alltoall", "gather"))
