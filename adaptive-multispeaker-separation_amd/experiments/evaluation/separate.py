# coding: utf-8
"""python -m experiments.evaluation.separate --model_folder ... --sortofmodel {STFT,front}[_enhanced]_{DPCL,L41}
       --input mix.wav --output_prefix out [--hop H] [--resample [--output_rate R] [--input_rate R]]

Separate one whole recording: the model's inference recipe (the same ones experiments/evaluation/eval.py uses) on overlapping chunks
of --chunk_size samples, the chunk outputs tracked across the chunk borders and cross-faded on the GPU (Network.separate_recording,
ams_hip/stitch.py).  Input: 16-bit PCM mono .wav at config.fs, or .npy float32 [N].  Output: <prefix>_<k>.wav (or .npy for an .npy
input), k = 0 .. nb_speakers - 1.  Without --resample there is no resampling and no channel mixing: anything else is refused.

With --clustering recording, --speakers auto (2 .. nb_speakers) or --speakers LO:HI chooses the number of speakers S_r of the recording
 and k = 0 .. S_r - 1 are written; LO = 1 needs --min_score X, the score below which the recording counts as one
speaker.

--clustering recording_soft is the recording-level mode of a model with a soft k-means (--beta_kmeans): one soft
k-means over the embeddings of all chunks, its soft labels as the masks.

With --resample the input may be a 16-bit PCM .wav of 1 .. 8 channels at any rate whose reduced ratio to config.fs has both terms in
1 .. 1024 (every standard rate from 11025 to 96000 Hz), or an .npy float32 [N] at --input_rate.  The frames are uploaded as they are;
decoding, the channel down-mix and the way to config.fs are one GPU kernel, the separated tracks go back to --output_rate (default: the
rate of the input) on the GPU as well (ams_hip/resample.py).  The outputs are mono."""
import wave

import numpy as np

import config


def build_parser():
    from utils.trainer import MyArgs
    p = MyArgs()
    p.parser.add_argument('--model_folder', help='Path to the Model folder to load', required=True)
    p.parser.add_argument('--sortofmodel', help='Sort of model', required=True)
    p.parser.add_argument('--input', help='Recording to separate: 16-bit PCM mono .wav at %d Hz, or .npy float32 [N]; with --resample a '
                          '16-bit PCM .wav of 1 .. 8 channels at any common rate, or .npy float32 [N] at --input_rate' % config.fs,
                          required=True)
    p.parser.add_argument('--output_prefix', help='Outputs are written to <prefix>_<k>.wav (.npy for an .npy input)', required=True)
    p.parser.add_argument('--hop', type=int, help='Samples between two chunks, ceil(chunk_size / 2) .. chunk_size - 1 '
                          '(default: half a chunk)', required=False, default=None)
    p.parser.add_argument('--resample', action='store_true', help='Accept another sample rate and several channels: mix down, resample '
                          'to %d Hz, separate, and resample the outputs back, all on the GPU' % config.fs)
    p.parser.add_argument('--output_rate', type=int, help='Sample rate of the outputs with --resample (default: the rate of the input)',
                          required=False, default=None)
    p.parser.add_argument('--input_rate', type=int, help='Sample rate of an .npy input (required with --resample and .npy)',
                          required=False, default=None)
    p.parser.add_argument('--clustering', choices=['chunk', 'recording', 'recording_soft'], default='chunk', help="k-means per chunk with "
                          "the outputs tracked across the chunk borders (default), or ONE k-means per recording over the embeddings of all "
                          "its chunks: 'recording' for a hard k-means (DESIGN.md 4.10), 'recording_soft' for a model with --beta_kmeans "
                          "(DESIGN.md 4.13)")
    add_speakers_args(p.parser)
    p.add_adapt_args()
    p.add_separator_args()
    return p


def add_speakers_args(parser):
    parser.add_argument('--speakers', help="With --clustering recording: choose every recording's number of speakers, 'auto' "
                        "(2 .. nb_speakers) or LO:HI (DESIGN.md 4.11); the tracks 0 .. S_r - 1 are written", required=False, default=None)
    parser.add_argument('--min_score', type=float, help='With --speakers 1:HI: the score below which a recording counts as one speaker '
                        '(no default: the criterion has not been measured on a trained model)', required=False, default=None)
    parser.add_argument('--recording_seeding', choices=['model', 'plusplus'], default='model', help="With --clustering recording or "
                        "recording_soft: the seeds of the recording's k-means are the model's uniform draw (default) or chosen on the GPU by "
                        "k-means++, D^2 sampling (DESIGN.md 4.14)")


def seeding_arg(args, whole=False):
    """--recording_seeding, refused with SystemExit before a model is built where no recording is clustered as a whole."""
    if args.recording_seeding == 'plusplus' and args.clustering == 'chunk' and not whole:
        raise SystemExit('--recording_seeding plusplus goes with --clustering recording or recording_soft')
    return args.recording_seeding


def speakers_arg(args):
    """--speakers / --min_score -> None or (lo, hi), refused with SystemExit before a model is built."""
    if args.speakers is None:
        if args.min_score is not None:
            raise SystemExit('--min_score goes with --speakers')
        return None
    from ams_hip import spk_count
    if args.clustering != 'recording':
        raise SystemExit('--speakers goes with --clustering recording: the count is chosen on the embeddings of a whole recording')
    if 'enhance' in args.sortofmodel:
        raise SystemExit('--speakers with --sortofmodel %s: choosing the count for a model with an enhance layer is not built'
                         % args.sortofmodel)
    try:
        lo, hi = spk_count.parse_speakers(args.speakers, args.nb_speakers)
        spk_count.check_range(lo, hi, args.nb_speakers, args.min_score)
    except ValueError as e:
        raise SystemExit('--speakers %s: %s' % (args.speakers, e))
    return lo, hi


def read_wav(path, fs=None):
    """16-bit PCM mono at fs (default config.fs) -> float32 [N] in [-1, 1): samples / 32768."""
    fs = config.fs if fs is None else fs
    with wave.open(path, 'rb') as w:
        if w.getnchannels() != 1:
            raise SystemExit('%s has %d channels: one channel only (mix them down first)' % (path, w.getnchannels()))
        if w.getsampwidth() != 2 or w.getcomptype() != 'NONE':
            raise SystemExit('%s is not 16-bit PCM (%d bytes per sample, compression %s)' % (path, w.getsampwidth(), w.getcomptype()))
        if w.getframerate() != fs:
            raise SystemExit('%s has a sample rate of %d Hz: the models work at %d Hz and nothing here resamples'
                             % (path, w.getframerate(), fs))
        raw = w.readframes(w.getnframes())
    return np.frombuffer(raw, dtype='<i2').astype(np.float32) / np.float32(32768.0)


def read_recording(path):
    """16-bit PCM of 1 .. 8 channels at any rate -> (int16 frames [N, CH], rate): the samples as the file has them, no arithmetic."""
    with wave.open(path, 'rb') as w:
        if w.getsampwidth() != 2 or w.getcomptype() != 'NONE':
            raise SystemExit('%s is not 16-bit PCM (%d bytes per sample, compression %s)' % (path, w.getsampwidth(), w.getcomptype()))
        if not 1 <= w.getnchannels() <= 8:
            raise SystemExit('%s has %d channels: 1 .. 8 channels can be mixed down' % (path, w.getnchannels()))
        channels, fs = w.getnchannels(), w.getframerate()
        raw = w.readframes(w.getnframes())
    return np.frombuffer(raw, dtype='<i2').reshape(-1, channels), fs


def write_wav(path, x, fs=None):
    """float32 [N] -> 16-bit PCM mono: round(x * 32768) clipped symmetrically to +-32767.  Non-finite samples are refused."""
    fs = config.fs if fs is None else fs
    if not np.all(np.isfinite(x)):
        raise SystemExit('%s: %d of %d samples are not finite; nothing written' % (path, int((~np.isfinite(x)).sum()), np.size(x)))
    pcm = np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32767, 32767).astype('<i2')
    with wave.open(path, 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(fs)
        w.writeframes(pcm.tobytes())


def read_input(path):
    if path.endswith('.npy'):
        x = np.load(path)
        if x.ndim != 1 or x.dtype != np.float32:
            raise SystemExit('%s holds %s %s: a float32 array [N] is expected' % (path, x.dtype, x.shape))
        return x
    return read_wav(path)


def write_outputs(prefix, out, as_npy, fs=None):
    paths = []
    for k, row in enumerate(np.asarray(out)):
        path = '%s_%d.%s' % (prefix, k, 'npy' if as_npy else 'wav')
        if as_npy:
            np.save(path, np.asarray(row, np.float32))
        else:
            write_wav(path, row, fs)
        paths.append(path)
    return paths


def main(argv=None):
    args = build_parser().get_args(argv)
    if 'pretraining' in args.sortofmodel:
        raise SystemExit('--sortofmodel %s: a pretraining model separates with masks made from the clean sources; a recording comes '
                         'without them' % args.sortofmodel)
    speakers = speakers_arg(args)
    seeding = seeding_arg(args)
    fs = out_fs = None
    if args.resample:
        from ams_hip import resample
        if args.input.endswith('.npy'):
            if args.input_rate is None:
                raise SystemExit('--resample with an .npy input needs --input_rate: an array carries no sample rate')
            x, fs = read_input(args.input), args.input_rate
        else:
            x, fs = read_recording(args.input)
            if args.input_rate not in (None, fs):
                raise SystemExit('--input_rate %d, but %s has a sample rate of %d Hz' % (args.input_rate, args.input, fs))
        out_fs = fs if args.output_rate is None else args.output_rate
        try:
            resample.ratio(fs, config.fs)
            resample.ratio(config.fs, out_fs)
        except ValueError as e:
            raise SystemExit('%s: %s' % (args.input, e))
    else:
        if args.output_rate is not None or args.input_rate is not None:
            raise SystemExit('--output_rate and --input_rate go with --resample')
        x = read_input(args.input)
    if x.shape[0] < 1:
        raise SystemExit('%s is empty' % args.input)
    from experiments.evaluation.eval import pick
    inferencer, sep = pick(args.sortofmodel)
    tr = inferencer(sep, 'inference', **vars(args))
    model = tr.prepare_inference()
    with tr.graph.as_default():
        out = model.separate_recording(x, hop=args.hop, fs=fs, output_fs=out_fs, clustering=args.clustering, speakers=speakers,
                                       min_score=args.min_score, recording_seeding=seeding).cpu().numpy()
    paths = write_outputs(args.output_prefix, out, args.input.endswith('.npy'), out_fs)
    print('\n'.join(paths))
    return paths


if __name__ == '__main__':
    main()
