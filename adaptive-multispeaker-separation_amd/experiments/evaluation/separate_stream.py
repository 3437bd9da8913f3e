# coding: utf-8
"""python -m experiments.evaluation.separate_stream --model_folder ... --sortofmodel {STFT,front}[_enhanced]_{DPCL,L41}
       (--inputs a.wav [b.wav ...] --output_dir D | --input - --format {s16le,f32le} --output_prefix P) [--block N] [--hop H]

Separate streams as they arrive: the inputs are read in blocks of --block samples (default: the hop) and pushed as parallel streams
through Network.open_streams (ams_hip/stream.py); what a push returns is written at once, one chunk behind the input.
--inputs: 16-bit PCM mono .wav files at config.fs, one stream each; the tracks go to D/<stem>_<k>.wav.  --input -: raw mono samples at
config.fs on standard input, little-endian 16-bit integers (s16le) or 32-bit floats (f32le); the tracks go to P_<k>.wav.  The .wav files
are written incrementally with experiments.evaluation.separate.write_wav's sample conversion, and their headers are fixed when a
stream ends.  There is no resampling, no channel mixing, no recording-level clustering and no speaker counting on a stream: those need
the whole recording, or are not built."""
import os
import sys
import wave

import numpy as np

import config
from experiments.evaluation import separate as one


def build_parser():
    from utils.trainer import MyArgs
    p = MyArgs()
    p.parser.add_argument('--model_folder', help='Path to the Model folder to load', required=True)
    p.parser.add_argument('--sortofmodel', help='Sort of model', required=True)
    p.parser.add_argument('--inputs', nargs='+', help='Streams to separate in parallel: 16-bit PCM mono .wav files at %d Hz' % config.fs,
                          required=False, default=None)
    p.parser.add_argument('--input', help="'-': one stream of raw mono samples at %d Hz on standard input (see --format)" % config.fs,
                          required=False, default=None)
    p.parser.add_argument('--format', choices=['s16le', 'f32le'], help='Sample format of --input -', required=False, default=None)
    p.parser.add_argument('--output_dir', help='With --inputs: the tracks are written to <output_dir>/<stem>_<k>.wav', required=False,
                          default=None)
    p.parser.add_argument('--output_prefix', help='With --input -: the tracks are written to <prefix>_<k>.wav', required=False, default=None)
    p.parser.add_argument('--block', type=int, help='Samples read and pushed per stream at a time (default: the hop)', required=False,
                          default=None)
    p.parser.add_argument('--hop', type=int, help='Samples between two chunks, ceil(chunk_size / 2) .. chunk_size - 1 '
                          '(default: half a chunk)', required=False, default=None)
    p.parser.add_argument('--resample', action='store_true', help='Refused: resampling a stream is not built')
    p.parser.add_argument('--clustering', default='chunk', help="Only 'chunk': the other modes need the whole recording")
    p.parser.add_argument('--speakers', help='Refused: counting speakers needs the whole recording', required=False, default=None)
    p.add_adapt_args()
    p.add_separator_args()
    return p


class WavBlocks(object):
    """A 16-bit PCM mono .wav at config.fs, read block by block: read(n) -> float32 [<= n], samples / 32768; empty at the end.  Anything
    else is refused with experiments.evaluation.separate.read_wav's words."""

    def __init__(self, path, fs=None):
        fs = config.fs if fs is None else fs
        self.path = path
        self.w = w = wave.open(path, 'rb')
        try:
            if w.getnchannels() != 1:
                raise SystemExit('%s has %d channels: one channel only (mix them down first)' % (path, w.getnchannels()))
            if w.getsampwidth() != 2 or w.getcomptype() != 'NONE':
                raise SystemExit('%s is not 16-bit PCM (%d bytes per sample, compression %s)' % (path, w.getsampwidth(), w.getcomptype()))
            if w.getframerate() != fs:
                raise SystemExit('%s has a sample rate of %d Hz: the models work at %d Hz and nothing here resamples'
                                 % (path, w.getframerate(), fs))
        except SystemExit:
            w.close()
            raise

    def read(self, n):
        raw = self.w.readframes(n)
        return np.frombuffer(raw, dtype='<i2').astype(np.float32) / np.float32(32768.0)

    def close(self):
        self.w.close()


class RawBlocks(object):
    """Raw mono samples from a binary file object (standard input): 's16le' -> samples / 32768, 'f32le' as they are.  read(n) returns
    fewer than n samples only at the end; bytes that do not make a whole sample there are refused."""

    def __init__(self, f, fmt):
        if fmt not in ('s16le', 'f32le'):
            raise SystemExit("--format %s: 's16le' or 'f32le'" % fmt)
        self.f, self.fmt, self.width = f, fmt, 2 if fmt == 's16le' else 4

    def read(self, n):
        want, parts = n * self.width, []
        while want > 0:
            raw = self.f.read(want)
            if not raw:
                break
            parts.append(raw)
            want -= len(raw)
        raw = b''.join(parts)
        if len(raw) % self.width:
            raise SystemExit('the input ends inside a sample: %d bytes left for samples of %d' % (len(raw) % self.width, self.width))
        if self.fmt == 's16le':
            return np.frombuffer(raw, dtype='<i2').astype(np.float32) / np.float32(32768.0)
        return np.frombuffer(raw, dtype='<f4').astype(np.float32)

    def close(self):
        pass


class WavTrack(object):
    """One 16-bit PCM mono .wav written piece by piece: write(x) converts as experiments.evaluation.separate.write_wav does
    (round(x * 32768) clipped symmetrically to +-32767, non-finite samples refused); close() fixes the header."""

    def __init__(self, path, fs=None):
        self.path, self.frames = path, 0
        self.w = wave.open(path, 'wb')
        self.w.setnchannels(1)
        self.w.setsampwidth(2)
        self.w.setframerate(config.fs if fs is None else fs)

    def write(self, x):
        x = np.asarray(x)
        if not np.all(np.isfinite(x)):
            raise SystemExit('%s: %d of %d samples are not finite; writing stopped after %d samples'
                             % (self.path, int((~np.isfinite(x)).sum()), np.size(x), self.frames))
        pcm = np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32767, 32767).astype('<i2')
        self.w.writeframesraw(pcm.tobytes())
        self.frames += pcm.shape[0]

    def close(self):
        self.w.close()                                             # (the wave module writes the final lengths into the header)


def run(sep, readers, tracks, block):
    """Reads `block` samples per open stream, pushes them together, writes what comes back; a stream whose reader is at its end is
    closed and its tracks are finished.  readers [n], tracks [n][S] -> the samples written per stream."""
    n = len(readers)
    live, written = [True] * n, [0] * n

    def put(s, out):
        out = out.cpu().numpy()
        for k, t in enumerate(tracks[s]):
            t.write(out[k])
        written[s] += out.shape[1]

    while any(live):
        blocks, ended = [None] * n, []
        for s in range(n):
            if live[s]:
                b = readers[s].read(block)
                if b.shape[0]:
                    blocks[s] = b
                else:
                    ended.append(s)
        if any(b is not None for b in blocks):
            outs = sep.push(blocks)
            for s in range(n):
                if blocks[s] is not None:
                    put(s, outs[s])
        for s in ended:
            put(s, sep.close(s))
            for t in tracks[s]:
                t.close()
            readers[s].close()
            live[s] = False
    return written


def check_args(args):
    """Every refusal that needs no model, as SystemExit -> ('files', paths) or ('stdin', None)."""
    if 'pretraining' in args.sortofmodel:
        raise SystemExit('--sortofmodel %s: a pretraining model separates with masks made from the clean sources; a stream comes '
                         'without them' % args.sortofmodel)
    if args.resample:
        raise SystemExit('--resample: not built for streams (it needs a resampler that carries its state from block to block); '
                         'bring the stream to %d Hz mono first' % config.fs)
    if args.clustering != 'chunk':
        raise SystemExit('--clustering %s: not built for streams: recording-level clustering needs the whole recording' % args.clustering)
    if args.speakers is not None:
        raise SystemExit('--speakers: not built for streams: the count is chosen on the embeddings of a whole recording')
    if (args.inputs is None) == (args.input is None):
        raise SystemExit('give either --inputs a.wav [b.wav ...] or --input -')
    if args.block is not None and args.block < 1:
        raise SystemExit('--block %d: at least one sample' % args.block)
    if args.inputs is not None:
        if args.output_dir is None or args.output_prefix is not None or args.format is not None:
            raise SystemExit('--inputs goes with --output_dir (and without --output_prefix and --format)')
        stems = [os.path.splitext(os.path.basename(p))[0] for p in args.inputs]
        for i, st in enumerate(stems):
            if st in stems[:i]:
                raise SystemExit('%s and %s would both be written as %s_<k>.wav: every input needs a file name of its own'
                                 % (args.inputs[stems.index(st)], args.inputs[i], st))
        for p in args.inputs:
            if not p.endswith('.wav'):
                raise SystemExit('%s: a stream from a file is a 16-bit PCM mono .wav' % p)
            WavBlocks(p).close()                                   # read_wav's refusals, before a model is built
        return 'files', list(args.inputs)
    if args.input != '-':
        raise SystemExit("--input %s: '-' (standard input) only; files are given with --inputs" % args.input)
    if args.format is None or args.output_prefix is None or args.output_dir is not None:
        raise SystemExit('--input - goes with --format and --output_prefix (and without --output_dir)')
    return 'stdin', None


def main(argv=None, stdin=None):
    args = build_parser().get_args(argv)
    kind, paths = check_args(args)
    from ams_hip import stitch
    L = int(args.chunk_size)
    H = stitch.default_hop(L) if args.hop is None else args.hop
    try:
        stitch.check_geometry(L, H)
    except ValueError as e:
        raise SystemExit('--hop %s: %s' % (args.hop, e))
    block = H if args.block is None else args.block
    from experiments.evaluation.eval import pick
    inferencer, sepr = pick(args.sortofmodel)
    tr = inferencer(sepr, 'inference', **vars(args))
    model = tr.prepare_inference()
    if kind == 'files':
        os.makedirs(args.output_dir, exist_ok=True)
        readers = [WavBlocks(p) for p in paths]
        prefixes = [os.path.join(args.output_dir, os.path.splitext(os.path.basename(p))[0]) for p in paths]
    else:
        readers = [RawBlocks(sys.stdin.buffer if stdin is None else stdin, args.format)]
        prefixes = [args.output_prefix]
    with tr.graph.as_default():
        sep = model.open_streams(len(readers), hop=H)
        names = [['%s_%d.wav' % (p, k) for k in range(sep.S)] for p in prefixes]
        tracks = [[WavTrack(nm) for nm in row] for row in names]
        run(sep, readers, tracks, block)
    out = [nm for row in names for nm in row]
    print('\n'.join(out))
    return out


if __name__ == '__main__':
    main()
