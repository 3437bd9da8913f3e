"""CPU: the boundary of the many-recordings stitcher -- ams_hip.stitch_batch.layout against the per-recording chunk arithmetic of
tests/stitch_ref.py, include/ams_stitch_batch.h against the exports of libams_stitch_batch.so (and the other libraries without its
symbols), the wrappers' refusal of CPU tensors, the refusals of experiments/evaluation/separate_many.py, and the kernels' resource usage
when compiled for gfx950."""
import ctypes
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest

from tests import stitch_ref as ref

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'adaptive-multispeaker-separation_amd')
NAMES = {'ams_stitchb_abi_version', 'ams_stitchb_chunks', 'ams_stitchb_workspace_bytes', 'ams_stitchb_stats', 'ams_stitchb_tracks',
         'ams_stitchb_ola'}


def _built(path):
    if not os.path.exists(path):
        import __graft_entry__
        __graft_entry__.build()
    return path


@pytest.mark.parametrize('L,H', [(256, 128), (250, 125), (256, 255), (2052, 1028), (20480, 10240)])
@pytest.mark.parametrize('S', [1, 2, 3, 6])
def test_layout_against_the_per_recording_arithmetic(L, H, S):
    from ams_hip import stitch_batch as sb
    n = [1, L - 1, L, L + 1, L + H, L + H + 1, 5 * L + 3, 2 * L, 1023, 1024, 1025]
    lay = sb.layout(n, L, H, S)
    R = len(n)
    assert (lay.R, lay.L, lay.H, lay.S) == (R, L, H, S)
    assert lay.n.dtype == lay.x_off.dtype == lay.out_off.dtype == lay.c_off.dtype == lay.blk_off.dtype == np.int64
    assert lay.chunk_rec.dtype == lay.blk_rec.dtype == np.int32
    C = [ref.nb_chunks(v, L, H) for v in n]
    assert lay.n.tolist() == n and lay.C.tolist() == C
    assert lay.c_off.tolist() == [sum(C[:r]) for r in range(R + 1)] and lay.Ctot == sum(C) >= R
    assert lay.chunk_rec.tolist() == [r for r in range(R) for _ in range(C[r])]
    blocks = [-(-v // 1024) for v in n]
    assert lay.blk_off.tolist() == [sum(blocks[:r]) for r in range(R + 1)] and lay.nblk == sum(blocks)
    assert lay.blk_rec.tolist() == [r for r in range(R) for _ in range(blocks[r])]
    # offsets: multiples of 4, in order, every recording and every output block clear of the next one
    assert np.all(lay.x_off % 4 == 0) and np.all(lay.out_off % 4 == 0) and lay.x_off[0] == 0 and lay.out_off[0] == 0
    ends_x = np.append(lay.x_off[1:], lay.x_total)
    ends_o = np.append(lay.out_off[1:], lay.out_total)
    assert np.all(lay.x_off + lay.n <= ends_x) and np.all(lay.out_off + S * lay.n <= ends_o)
    assert lay.x_total < sum(n) + 4 * R and lay.out_total < S * sum(n) + 4 * S * R        # and no more padding than alignment asks for
    assert [(s.start, s.stop) for s in map(lay.rec_chunks, range(R))] == list(zip(lay.c_off[:-1], lay.c_off[1:]))


def test_layout_defaults_and_refusals():
    from ams_hip import stitch_batch as sb
    lay = sb.layout([700], 256)
    assert (lay.H, lay.S, lay.Ctot, lay.C.tolist()) == (128, None, ref.nb_chunks(700, 256, 128), [5])
    assert lay.set_sources(3).out_off.tolist() == [0] and lay.out_total == 3 * 700
    with pytest.raises(ValueError):
        lay.set_sources(2)                                         # a layout keeps its number of sources
    for bad in ([], [0], [5, -1]):
        with pytest.raises(ValueError):
            sb.layout(bad, 256, 128, 2)
    for h in (127, 256):
        with pytest.raises(ValueError):
            sb.layout([700], 256, h, 2)
    for s in (0, 7):
        with pytest.raises(ValueError):
            sb.layout([700], 256, 128, s)
    # the seeded workload of tools/stitch_many_bench.py: 1483 chunks, 24 full passes of 64 instead of 256
    n = np.random.RandomState(7).randint(32000, 96001, size=256)
    lay = sb.layout(n, 20480, 10240, 2)
    assert lay.Ctot == 1483 and -(-lay.Ctot // 64) == 24


def test_header_and_exports():
    src = open(os.path.join(ROOT, 'include', 'ams_stitch_batch.h')).read()
    src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
    assert set(re.findall(r'\b(ams_\w+)\s*\(', src)) == NAMES
    from ams_hip import _lib, stitch, stitch_batch
    assert set(_lib.parse_header(stitch_batch.HEADER_PATH)) == NAMES
    path = _built(stitch_batch.LIB_PATH)
    out = subprocess.run(['nm', '-D', '--defined-only', path], capture_output=True, text=True, check=True).stdout
    exported = set(ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('ams_'))
    assert exported == NAMES
    lib = ctypes.CDLL(path)
    assert lib.ams_stitchb_abi_version() == 1 == stitch_batch.ABI_VERSION
    lib.ams_stitchb_workspace_bytes.restype = ctypes.c_size_t
    assert lib.ams_stitchb_workspace_bytes(1483, 2, 20480, 10240) == 1483 * 10 * 4 * 4
    assert lib.ams_stitchb_workspace_bytes(3, 6, 4100, 2050) == 3 * 3 * 36 * 4
    assert lib.ams_stitchb_workspace_bytes(1, 2, 256, 128) == 16                      # one chunk is valid here: a row of zeros
    assert lib.ams_stitchb_workspace_bytes(0, 2, 256, 128) == 0 and lib.ams_stitchb_workspace_bytes(3, 7, 256, 128) == 0
    assert lib.ams_stitchb_workspace_bytes(3, 2, 256, 127) == 0
    for other in (stitch.LIB_PATH, _lib.LIB_PATH):                                    # the other libraries gained nothing
        syms = subprocess.run(['nm', '-D', '--defined-only', _built(other)], capture_output=True, text=True, check=True).stdout
        assert 'ams_stitchb_' not in syms, other
    assert 'stitchb' not in open(stitch.HEADER_PATH).read() and 'stitchb' not in open(_lib.HEADER_PATH).read()


def test_wrappers_refuse_cpu_tensors():
    from ams_hip import stitch_batch as sb
    from ams_hip._lib import AmsError
    lay = sb.layout([700, 100], 256, 128, 2)
    est = torch.zeros(lay.Ctot, 2, 256)
    with pytest.raises(AmsError):
        sb.chunks_many([torch.zeros(700), torch.zeros(100)], 256, 128)
    with pytest.raises(AmsError):
        sb.chunks_packed(torch.zeros(lay.x_total), lay)
    with pytest.raises(AmsError):
        sb.border_stats_many(est, lay)
    with pytest.raises(AmsError):
        sb.tracks_many(torch.zeros(lay.Ctot, 2, 2), lay)
    with pytest.raises(AmsError):
        sb.overlap_add_many(est, torch.zeros(lay.Ctot, 2, dtype=torch.int32), lay)
    with pytest.raises(AmsError):
        sb.stitch_many(est, lay)
    with pytest.raises(ValueError):
        sb.chunks_many([], 256, 128)


def _write_wav(path, pcm, fs, channels=1):
    with wave.open(path, 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(np.asarray(pcm, '<i2').tobytes())


def test_cli_flags_and_refusals(tmp_path):
    import config
    from experiments.evaluation import separate_many as cli
    base = ['--model_folder', 'm', '--sortofmodel', 'front_DPCL', '--output_dir', str(tmp_path / 'o')]
    a = cli.build_parser().get_args(base + ['--inputs', 'a.wav', 'b.wav', '--hop', '12000', '--nb_speakers', '3'])
    assert (a.inputs, a.input_list, a.output_dir, a.hop, a.nb_speakers, a.resample, a.output_rate) == \
        (['a.wav', 'b.wav'], None, str(tmp_path / 'o'), 12000, 3, False, None)
    assert cli.input_paths(a) == ['a.wav', 'b.wav']
    with pytest.raises(SystemExit):
        cli.build_parser().get_args(['--model_folder', 'm', '--sortofmodel', 's', '--inputs', 'a.wav'])        # no --output_dir

    pcm = np.random.RandomState(5).randint(-32768, 32768, size=1234).astype(np.int16)
    good, other, slow, empty = (str(tmp_path / n) for n in ('good.wav', 'other.wav', 'slow.wav', 'empty.wav'))
    _write_wav(good, pcm, config.fs)
    _write_wav(other, pcm[:1000], config.fs)
    _write_wav(slow, pcm, 2 * config.fs)
    _write_wav(empty, pcm[:0], config.fs)
    lst = str(tmp_path / 'list.txt')
    with open(lst, 'w') as f:
        f.write('%s\n\n%s\n' % (good, other))
    a = cli.build_parser().get_args(base + ['--input_list', lst])
    assert cli.input_paths(a) == [good, other]
    recs = cli.read_all([good, other], False)
    assert [x.shape for x, _ in recs] == [(1234,), (1000,)] and recs[0][0].dtype == np.float32 and recs[0][1] == config.fs
    recs = cli.read_all([good, slow], True)                        # with --resample: the frames as they are, each at its own rate
    assert [(x.shape, x.dtype, fs) for x, fs in recs] == [((1234, 1), np.int16, config.fs), ((1234, 1), np.int16, 2 * config.fs)]

    def refused(extra, *words):
        with pytest.raises(SystemExit) as e:                       # each before a model is built: 'm' is no model folder
            cli.main(base + extra)
        for w in words:
            assert w in str(e.value), (w, str(e.value))

    refused([], '--inputs')                                        # neither --inputs nor --input_list
    refused(['--inputs', good, '--input_list', lst], '--inputs')   # both
    os.makedirs(str(tmp_path / 'sub'))
    twin = str(tmp_path / 'sub' / 'good.wav')
    _write_wav(twin, pcm, config.fs)
    refused(['--inputs', good, other, twin], 'good', 'file name of its own')          # duplicate stems
    refused(['--inputs', good, str(tmp_path / 'good.npy')], 'good')                   # ... whatever the extension
    refused(['--inputs', good, empty], 'empty.wav is empty')
    refused(['--inputs', good, slow], 'differing sample rates', '--resample')
    refused(['--inputs', slow], 'sample rate')                     # one rate, but not the models': separate.read_wav's refusal
    refused(['--inputs', good, '--output_rate', '16000'], '--resample')
    refused(['--inputs', str(tmp_path / 'x.npy'), '--resample'], '.npy')
    nolist = str(tmp_path / 'nolist.txt')
    open(nolist, 'w').close()
    refused(['--input_list', nolist], 'names no input')
    with pytest.raises(SystemExit) as e:
        cli.main(['--model_folder', 'm', '--sortofmodel', 'pretraining', '--inputs', 'missing.wav', '--output_dir', 'o'])
    assert 'pretraining' in str(e.value) and 'clean sources' in str(e.value)
    assert not os.path.exists(str(tmp_path / 'o'))


def test_stitch_batch_kernels_compile_for_gfx950_without_scratch():
    """tools/kernel_resources.py on csrc/stitch/stitch_batch.hip with the library's flags: the same nineteen kernels as stitch.hip, no
    scratch, no spill, no warning; the gather and the cross-fade use no LDS."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'kernel_resources.py'),
                          os.path.join(PKG, 'csrc', 'stitch', 'stitch_batch.hip'), '-ffp-contract=off'],
                         capture_output=True, text=True, check=True)
    assert 'warning' not in run.stderr
    out = run.stdout.splitlines()[1:]
    names = ' '.join(out)
    for S in range(1, 7):
        for vec in ('true', 'false'):
            assert 'stats_kernel<%d, %s>' % (S, vec) in names, (S, vec)
    for k in ('chunks_kernel<true>', 'chunks_kernel<false>', 'ola_kernel<true>', 'ola_kernel<false>', 'stats_fold_kernel',
              'border_perm_kernel', 'tracks_kernel'):
        assert k in names, k
    rows = [ln.split() for ln in out if ln.strip()]
    assert len(rows) == 12 + 7
    for r in rows:
        vgpr, agpr, spill, scratch, occ, lds = r[-6:]
        assert spill == '0' and scratch == '0', r
        if 'chunks_kernel' in ' '.join(r) or 'ola_kernel' in ' '.join(r):
            assert lds == '0', r
