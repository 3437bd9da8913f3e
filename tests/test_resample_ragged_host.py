"""CPU: the boundary of the ragged resampler -- include/ams_resample_ragged.h against the exports of libams_resample_ragged.so (and
libams_resample.so with exactly its own header's names), the host tables against a numpy restatement, every limit of the header (all
returned before anything is launched), the wrappers' and separate_recordings' refusals (raised before any device work), the command
line's flag, and the kernels' resources."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
NAMES = {'ams_rsr_abi_version', 'ams_rsr_tiles', 'ams_rsr_tables', 'ams_rsr_run_pcm16', 'ams_rsr_run_f32'}
INVALID = -1
W = 12                                                             # words per job record
SRC, N_IN, ROWS, X_STRIDE, CHANNELS, UP, DOWN, TAP_OFF, DST, Y_STRIDE, N_KEEP, RESERVED = range(W)


def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


def _exports(path):
    out = subprocess.run(['nm', '-D', '--defined-only', _built(path)], capture_output=True, text=True, check=True).stdout
    return set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))


def _lib():
    from ams_hip import _lib, resample_ragged as rr
    lib = ctypes.CDLL(_built(rr.LIB_PATH))
    for name, (ret, argtypes) in _lib.parse_header(rr.HEADER_PATH).items():
        getattr(lib, name).restype, getattr(lib, name).argtypes = ret, argtypes
    return lib


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_header_and_exports():
    from ams_hip import _lib, resample, resample_ragged as rr
    src = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', 'ams_resample_ragged.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    assert set(_lib.parse_header(rr.HEADER_PATH)) == NAMES
    assert _exports(rr.LIB_PATH) == NAMES
    assert ctypes.CDLL(rr.LIB_PATH).ams_rsr_abi_version() == 1 == rr.ABI_VERSION
    # libams_resample.so: exactly its own header's names, as before the shared core existed
    want = set(_lib.parse_header(resample.HEADER_PATH))
    assert want == {'ams_resample_abi_version', 'ams_resample_out_len', 'ams_resample_pcm16', 'ams_resample_f32'}
    assert _exports(resample.LIB_PATH) == want
    assert ctypes.CDLL(resample.LIB_PATH).ams_resample_abi_version() == 1
    # no other library gained a ragged-resampler name
    others = [p for p in glob.glob(os.path.join(PKG, 'ams_hip', 'libams_*.so')) if os.path.basename(p) != 'libams_resample_ragged.so']
    assert len(others) >= 7
    for p in others:
        assert not any(n.startswith('ams_rsr_') for n in _exports(p)), p
    assert 'rsr' not in open(resample.HEADER_PATH).read() and 'rsr' not in open(_lib.HEADER_PATH).read()


def _jobs():
    """rows 1, 2 and 6; n_keep in {1, 255, 256, 257, M}; the pairs (1, 1), (1, 2), (441, 80), (1, 20).  float32 rows."""
    jobs, taps_len, dst = [], 0, 0
    where = {}
    for up, down in ((1, 1), (1, 2), (441, 80), (1, 20)):
        if up != down:
            where[(up, down)] = taps_len
            taps_len += 20 * max(up, down) + 1
    k = 0
    for up, down in ((1, 1), (1, 2), (441, 80), (1, 20)):
        for rows in (1, 2, 6):
            n_in = 6000 * down // up + 17 + k
            M = -((-n_in * up) // down)
            assert M > 257
            for n_keep in (1, 255, 256, 257, M):
                x_stride, y_stride = n_in + k % 3, n_keep + k % 2
                jobs.append([4 * (1000 * k), n_in, rows, x_stride, 0, up, down, where.get((up, down), 5), dst, y_stride, n_keep, 0])
                dst += rows * y_stride
                k += 1
    return np.asarray(jobs, np.int64), taps_len, dst


def test_host_tables_against_numpy():
    lib = _lib()
    jobs, taps_len, _ = _jobs()
    J = jobs.shape[0]
    assert J == 4 * 3 * 5
    # the restatement: ceil(n_keep / 256) tiles per row, rows of them per job, a running sum in front; the records behind it
    per_row = -(-jobs[:, N_KEEP] // 256)
    prefix = np.concatenate([[0], np.cumsum(jobs[:, ROWS] * per_row)])
    rec = jobs.copy()
    rec[:, RESERVED] = per_row
    rec[jobs[:, UP] == jobs[:, DOWN], TAP_OFF] = 0
    assert lib.ams_rsr_tiles(_ptr(jobs), J, taps_len) == prefix[-1]
    table = np.full((J + 1) + W * J, -7, np.int64)
    assert lib.ams_rsr_tables(_ptr(jobs), J, taps_len, _ptr(table)) == 0
    assert table[:J + 1].tolist() == prefix.tolist()
    assert np.array_equal(table[J + 1:].reshape(J, W), rec)
    # table memory is proportional to the jobs: the same words for signals a thousand times as long
    long_jobs = jobs.copy()
    long_jobs[:, N_IN] *= 1000
    long_jobs[:, X_STRIDE] *= 1000
    assert lib.ams_rsr_tables(_ptr(long_jobs), J, taps_len, _ptr(table)) == 0
    # the binding builds the same
    from ams_hip import resample_ragged as rr
    j2, t2 = rr.tables(jobs.tolist(), taps_len)
    assert np.array_equal(j2, jobs) and t2[:J + 1].tolist() == prefix.tolist() and np.array_equal(t2[J + 1:].reshape(J, W), rec)
    assert rr.job(8, 7001, 80, 441, 12, rows=2, n_keep=1000) == [8, 7001, 2, 7001, 0, 80, 441, 0, 12, 1000, 1000, 0]
    assert rr.job(0, 10, 2, 1, 0)[N_KEEP] == 20


def test_every_limit_is_invalid_arg_before_any_launch():
    from ams_hip import resample_ragged as rr
    lib = _lib()
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)                          # a host pointer: never dereferenced by a call that is refused
    taps_len = 20 * 441 + 1
    good = [0, 1000, 2, 1000, 0, 80, 441, 0, 0, 182, 182, 0]      # M = ceil(80 000 / 441) = 182
    big = 1 << 40

    def calls(job, J=1, tl=taps_len, y_len=big, pcm=None, jobs_null=False):
        j = np.asarray([job] * max(J, 1), np.int64)
        jp = None if jobs_null else _ptr(j)
        table = np.zeros((max(J, 1) + 1) + W * max(J, 1), np.int64)
        pcm = job[CHANNELS] >= 1 if pcm is None else pcm
        run = lib.ams_rsr_run_pcm16 if pcm else lib.ams_rsr_run_f32
        return (lib.ams_rsr_tiles(jp, J, tl), lib.ams_rsr_tables(jp, J, tl, _ptr(table)), run(p, p, tl, jp, J, p, p, y_len, None))

    def edit(**kw):
        j = list(good)
        for k, v in kw.items():
            j[globals()[k]] = v
        return j
    assert lib.ams_rsr_tiles(_ptr(np.asarray([good], np.int64)), 1, taps_len) == 2
    table = np.zeros(2 + W, np.int64)
    assert lib.ams_rsr_tables(_ptr(np.asarray([good], np.int64)), 1, taps_len, _ptr(table)) == 0
    bad = [
        ('J < 1', dict(job=good, J=0)), ('J < 0', dict(job=good, J=-1)), ('NULL jobs', dict(job=good, jobs_null=True)),
        ('up 0', dict(job=edit(UP=0))), ('up 1025', dict(job=edit(UP=1025, DOWN=1))), ('down 0', dict(job=edit(DOWN=0))),
        ('down 1025', dict(job=edit(UP=1, DOWN=1025))), ('not coprime', dict(job=edit(UP=2, DOWN=4))), ('up = down = 2', dict(job=edit(UP=2, DOWN=2))),
        ('channels -1', dict(job=edit(CHANNELS=-1))), ('channels 9', dict(job=edit(CHANNELS=9, ROWS=1))),
        ('int16 frames with rows', dict(job=edit(CHANNELS=2, ROWS=2))),
        ('n_in 0', dict(job=edit(N_IN=0))), ('rows 0', dict(job=edit(ROWS=0))),
        ('M > 2^38', dict(job=edit(N_IN=(1 << 38) // 2 + 1, X_STRIDE=1 << 38, UP=2, DOWN=1, N_KEEP=5, Y_STRIDE=5), tl=41)),
        ('n_keep 0', dict(job=edit(N_KEEP=0))), ('n_keep M + 1', dict(job=edit(N_KEEP=183, Y_STRIDE=183))),
        ('x_stride short', dict(job=edit(X_STRIDE=999))), ('y_stride short', dict(job=edit(Y_STRIDE=181))),
        ('dst < 0', dict(job=edit(DST=-1))), ('src odd', dict(job=edit(SRC=2))),
        ('tap offset < 0', dict(job=edit(TAP_OFF=-1))), ('taps do not fit', dict(job=edit(TAP_OFF=1))),
        ('tap buffer short', dict(job=good, tl=taps_len - 1)), ('no taps', dict(job=good, tl=0)),
        ('2^31 tiles', dict(job=edit(N_IN=1 << 38, X_STRIDE=1 << 38, UP=1, DOWN=1, N_KEEP=1 << 38, Y_STRIDE=1 << 38, ROWS=2))),
    ]
    for what, kw in bad:
        assert calls(**kw) == (-1, INVALID, INVALID), what
    # the same job with one row is 2^30 tiles: inside the limits (nothing is launched here: the run call is not made)
    one = edit(N_IN=1 << 38, X_STRIDE=1 << 38, UP=1, DOWN=1, N_KEEP=1 << 38, Y_STRIDE=1 << 38, ROWS=1)
    assert lib.ams_rsr_tiles(_ptr(np.asarray([one], np.int64)), 1, 1) == 1 << 30
    # what only the run calls can see: NULL pointers, the other kind of input, rows that leave y
    j = np.asarray([good], np.int64)
    for args in ((None, p, p, p, p), (p, None, p, p, p), (p, p, None, p, p), (p, p, p, None, p), (p, p, p, p, None)):
        x, taps, jp, tab, y = args
        assert lib.ams_rsr_run_f32(x, taps, taps_len, _ptr(j) if jp else None, 1, tab, y, big, None) == INVALID, args
    assert lib.ams_rsr_tables(_ptr(j), 1, taps_len, None) == INVALID
    assert lib.ams_rsr_run_pcm16(p, p, taps_len, _ptr(j), 1, p, p, big, None) == INVALID                    # float32 rows to the int16 call
    jp = np.asarray([edit(CHANNELS=2, ROWS=1)], np.int64)
    assert lib.ams_rsr_run_f32(p, p, taps_len, _ptr(jp), 1, p, p, big, None) == INVALID                     # int16 frames to the float32 call
    for y_len in (0, 181, 182, 182 + 181):                                                                  # two rows of 182, stride 182
        assert lib.ams_rsr_run_f32(p, p, taps_len, _ptr(j), 1, p, p, y_len, None) == INVALID, y_len
    # the binding says the same as an AmsError, without a device
    from ams_hip._lib import AmsError
    with pytest.raises(AmsError, match='ams_rsr_tables'):
        rr.tables([edit(N_KEEP=183, Y_STRIDE=183)], taps_len)
    with pytest.raises(AmsError, match='ams_rsr_tables'):
        rr.tables([], taps_len)


def test_the_wrappers_refuse_cpu_tensors_and_bad_lists():
    from ams_hip import resample_ragged as rr
    from ams_hip import stitch_batch as sb
    from ams_hip._lib import AmsError
    lay = sb.layout([1271, 500], 2048, 1024, 2)
    with pytest.raises(AmsError, match='device tensors'):
        rr.from_model_rate(torch.zeros(lay.out_total), lay, 2, [44100, 16000], [7001, 1000])
    with pytest.raises(AmsError, match='device tensors'):
        rr.run(torch.zeros(10), False, torch.zeros(41), [rr.job(0, 10, 2, 1, 0)], torch.zeros(20))
    x = np.zeros(1000, np.float32)
    f = np.zeros((1000, 2), np.int16)
    for recs, fs, word in (([x, x], [8000], 'sample rates'), ([], [], 'at least one'), ([x, x], [8000, 22051], 'recording 1'),
                           ([x, f], [8000, 8000], 'all int16'), ([x.astype(np.float64)], [8000], 'all int16'),
                           ([np.zeros((10, 9), np.int16)], [8000], '1 .. 8 channels'), ([np.zeros((10, 0), np.int16)], [8000], 'channels'),
                           ([f, np.zeros((0, 2), np.int16)], [8000, 8000], 'recording 1.*at least one sample'),
                           ([x, np.zeros((4, 4), np.float32)], [8000, 8000], 'recording 1')):
        with pytest.raises(ValueError, match=word):
            rr.to_model_rate(recs, fs, L=2048, H=1024, S=2, fs_model=8000)
    for rows, fs, n, word in ((2, [44100], [5, 5], 'row counts'), ([2, 3], [44100, 8000], [5, 5], 'recording 1.*rows'),
                              (2, [44100, 22051], [5, 5], 'recording 1'), (2, [44100, 16000], [7008, 5], 'recording 0.*asked for 7008'),
                              (2, [44100, 16000], [7001, 0], 'recording 1.*asked for 0')):
        with pytest.raises(ValueError, match=word):
            rr.from_model_rate(torch.zeros(lay.out_total), lay, rows, fs, n, fs_model=8000)
    assert rr.model_lengths([7001, 9000, 2100], [16000, 44100, 8000], 8000) == [3501, 1633, 2100]


def _stub():
    from tests.test_kmeans_ragged_host import _stub as stub
    return stub()


def test_separate_recordings_refuses_bad_rates_before_any_device_work():
    x = np.zeros(5000, np.float32)
    f = np.zeros((5000, 2), np.int16)
    for xs in ([x, x], [f, f]):
        with pytest.raises(ValueError, match='fs has 3 rates for 2 recordings'):
            _stub().separate_recordings(xs, fs=[8000, 16000, 44100])
        with pytest.raises(ValueError, match='recording 1'):
            _stub().separate_recordings(xs, fs=[16000, 22051])
        with pytest.raises(ValueError, match='recording 1'):
            _stub().separate_recordings(xs, fs=16000, output_fs=[16000, 22051])
        with pytest.raises(ValueError, match='output_fs has 1 rates for 2 recordings'):
            _stub().separate_recordings(xs, fs=[16000, 44100], output_fs=[8000])
        for bad in ([16000, 44100.5], [16000, '44100'], [16000, None], 16000.5):
            with pytest.raises(ValueError, match='a sample rate is an integer'):
                _stub().separate_recordings(xs, fs=bad)
        with pytest.raises(ValueError, match='a sample rate is an integer'):
            _stub().separate_recordings(xs, fs=[16000, 44100], output_fs=[8000, 1.5])
    # the scalar form keeps the resampler's own words (no recording is named)
    with pytest.raises(ValueError) as e:
        _stub().separate_recordings([x, x], fs=22051)
    assert 'recording' not in str(e.value) and '22051' in str(e.value)
    with pytest.raises(ValueError, match='one dtype'):
        _stub().separate_recordings([x, f], fs=[16000, 16000])


def test_the_command_line_takes_one_stream_with_resample_only():
    from experiments.evaluation import separate_many
    base = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--inputs', 'a.wav', '--output_dir', 'o']
    assert separate_many.build_parser().get_args(base).one_stream is False
    assert separate_many.build_parser().get_args(base + ['--resample', '--one_stream']).one_stream is True
    with pytest.raises(SystemExit, match='--resample'):
        separate_many.main(base + ['--one_stream'])


def test_kernels_keep_their_state_in_registers():
    """tools/kernel_resources.py on csrc/resample/resample_ragged.hip with the library's flags: one kernel per kind of input, no scratch,
    no spill, no warning; the 16 KB of LDS of the decimating arm."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'),
                          os.path.join(PKG, 'csrc', 'resample', 'resample_ragged.hip')], capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    rows = [ln.split() for ln in run.stdout.splitlines()[1:] if ln.strip()]
    names = ' '.join(' '.join(r) for r in rows)
    for k in ('ragged_kernel<Pcm16Source>', 'ragged_kernel<F32Source>'):
        assert k in names, k
    assert len(rows) == 2
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0' and lds == '16384', r
