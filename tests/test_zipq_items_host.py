"""The work items of k_zipqp_f32 and how its workgroups walk them (contractn_amd/csrc/zipq_items.h) - on the CPU under
AddressSanitizer + UBSan.

`make -C contractn_amd/csrc zipq_check` builds the header and a stand-alone driver (zipq_check.cpp).  The same inline
functions size the grid in the engine and drive the item loop in the kernel.  For every `items` in 1 .. 2,100 and every
`grid` of GRIDS with grid <= items the driver walks every block id as the kernel does and checks that

  * the XCD remap is a permutation of 0 .. grid - 1;
  * every item is walked exactly once;
  * a workgroup's rounds number ceil or floor of items / grid;
  * for an even grid, items 2 r and 2 r + 1 - the two 128-u blocks of a |u| = 256 replica - fall in the same round.

A few walks are dumped and checked here once more, and the grid cap is clamped to [1, n_cu]."""
import os
import subprocess

import pytest

from tests.helpers import ROOT

CSRC = os.path.join(ROOT, "contractn_amd", "csrc")
BINARY = os.path.join(ROOT, "contractn_amd", "lib", "zipq_check_asan")
GRIDS = (1, 2, 3, 7, 8, 9, 255, 256, 304)
MAX_ITEMS = 2100


@pytest.fixture(scope="module")
def binary():
    proc = subprocess.run(["make", "-C", CSRC, "zipq_check"], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr[-3000:]
    assert os.path.exists(BINARY)
    return BINARY


def run(binary, texts):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    proc = subprocess.run([binary], input="\n".join(texts) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert proc.stderr == "", proc.stderr[-4000:]
    lines = proc.stdout.strip().splitlines()
    assert len(lines) == len(texts), proc.stdout[-2000:]
    assert proc.returncode == 0, proc.stdout[-2000:]
    return lines


def test_every_items_and_grid_walks_every_item_once(binary):
    cases = [(items, grid) for items in range(1, MAX_ITEMS + 1) for grid in GRIDS if grid <= items]
    lines = run(binary, ["walk %d %d" % c for c in cases])
    for (items, grid), line in zip(cases, lines):
        assert line == "items=%d grid=%d perm=ok once=ok rounds=ok pair=ok ok" % (items, grid), line


@pytest.mark.parametrize("items,grid", [(9, 2), (9, 4), (3, 1), (1024, 256), (2100, 304), (517, 255), (1, 1), (10, 9)])
def test_dumped_walks(binary, items, grid):
    (line,) = run(binary, ["dump %d %d" % (items, grid)])
    pids, walked = [], []
    for bid, entry in enumerate(line.split()):
        b, pid, its = entry.split(":")
        its = [int(i) for i in its.split(",")] if its else []
        assert int(b) == bid and its == list(range(int(pid), items, grid)), entry
        assert len(its) in (items // grid, -(-items // grid))
        pids.append(int(pid))
        walked += its
    assert sorted(pids) == list(range(grid)) and sorted(walked) == list(range(items))
    # consecutive pids share an XCD: block ids bid, bid + 8, ... are consecutive pids
    for bid in range(grid - 8):
        assert pids[bid + 8] == pids[bid] + 1
    if grid % 2 == 0:
        rounds = {i: i // grid for i in range(items)}
        assert all(rounds[i] == rounds[i + 1] for i in range(0, items - 1, 2))


def test_the_cap_is_clamped_and_the_grid_never_exceeds_items_or_cus(binary):
    n_cu = 256
    caps = [-5, 0, 1, 2, 3, 255, 256, 257, 1000, 1 << 30]
    itemses = [1, 2, 3, 255, 256, 257, 511, 512, 1024]
    lines = run(binary, ["grid %d %d %d" % (items, n_cu, cap) for cap in caps for items in itemses])
    it = iter(lines)
    for cap in caps:
        want_cap = n_cu if cap <= 0 else min(max(cap, 1), n_cu)
        for items in itemses:
            assert next(it) == "cap=%d grid=%d" % (want_cap, min(items, want_cap)), (cap, items)
    assert run(binary, ["grid 1024 304 0", "grid 1024 304 400", "grid 5 0 0"]) == ["cap=304 grid=304", "cap=304 grid=304", "cap=1 grid=1"]


def test_replica_and_u_block_of_an_item(binary):
    cases = [(item, per) for per in (1, 2, 3) for item in range(0, 13)]
    lines = run(binary, ["rt %d %d" % c for c in cases])
    for (item, per), line in zip(cases, lines):
        assert line == "r=%d t=%d" % (item // per, item % per)
