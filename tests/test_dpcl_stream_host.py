"""CPU: the work geometry of the streamed E = 40 loss backward (csrc/dpcl.hip: dpcl_bwd_u2_kernel<E, S, D>), recomputed for the
benchmark shape, and what the compiler made of the kernel.  No GPU call."""
import ctypes
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')

CUS = 256                   # MI355X
LDS_PER_CU = 160 * 1024
VGPR_PER_SIMD = 512         # per lane: a wave of 4 per SIMD may use 128
B, TF, E, S = 64, 20480, 40, 2          # bench.py's step: 64 utterances x 20480 points


def _geometry():
    from ams_hip import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    g = (ctypes.c_int * 5)()
    _lib.load().ams_dpcl_stream_geometry(g)
    return tuple(g)


def _resources():
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'), os.path.join(PKG, 'csrc', 'dpcl.hip'),
                          'dpcl_bwd_u2_kernel'], capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    rows = {}
    for ln in run.stdout.splitlines()[1:]:
        name, rest = ln.rsplit('>', 1)
        rows[name.split('<')[1].replace(' ', '')] = [int(x) for x in rest.split()]      # 'E,S,D' -> VGPR AGPR spill scratch occ LDS
    return rows


def test_the_benchmark_launch_is_a_whole_number_of_rounds():
    bch, depth, wgs, grp, waves = _geometry()
    grid = -(-TF // bch) * B
    slots = CUS * wgs
    assert TF % bch == 0 and grid % slots == 0, (grid, slots)      # no short last chunk, no partly filled last round
    assert bch % (grp * waves) == 0                                 # every wave of a full chunk walks the same number of groups
    # a CU's resident waves keep at least 64 KB of loads in flight: U rows, labels and 1/|u| of `depth` groups per wave
    in_flight = wgs * waves * depth * grp * 4 * (E + S + 1)
    assert in_flight >= 64 * 1024, in_flight


def test_the_stated_residency_is_what_the_compiler_gives():
    """No scratch, no spill; registers and LDS of the streamed arms admit the workgroups per CU the geometry counts on."""
    bch, depth, wgs, grp, waves = _geometry()
    rows = _resources()
    assert sorted(rows) == sorted(['40,%d,%d' % (s, d) for s in (2, 3) for d in (0, depth)])
    for key, (vgpr, agpr, spill, scratch, occ, lds) in rows.items():
        assert spill == 0 and scratch == 0, key
        if key.endswith(',%d' % depth):
            regs = -(-(vgpr + agpr) // 8) * 8                       # allocation granule
            assert wgs * waves // 4 * regs <= VGPR_PER_SIMD, (key, vgpr, agpr)
            assert wgs * lds <= LDS_PER_CU and lds >= waves * depth * (3 * 1024 + 512), (key, lds)
            assert occ == wgs * waves // 4, (key, occ)
