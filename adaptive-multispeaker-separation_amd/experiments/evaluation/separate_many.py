# coding: utf-8
"""python -m experiments.evaluation.separate_many --model_folder ... --sortofmodel {STFT,front}[_enhanced]_{DPCL,L41}
       (--inputs a.wav b.wav ... | --input_list file) --output_dir D [--hop H] [--resample [--output_rate R]]

Separate many recordings in one call: the chunks of all of them go through the model as one stream of full batches, and they are cut,
tracked and cross-faded by kernels whose launch count does not depend on the number of recordings (Network.separate_recordings,
ams_hip/stitch_batch.py).  Inputs as for experiments.evaluation.separate, whose .wav and .npy helpers are used here:
16-bit PCM mono .wav at config.fs, or .npy float32 [N]; --input_list names a text file with one path per line.  Output:
D/<stem>_<k>.wav (.npy for an .npy input), k = 0 .. nb_speakers - 1, where <stem> is the input's file name without its extension --
two inputs with one stem are refused.

With --resample the inputs are 16-bit PCM .wav files of 1 .. 8 channels at any common rate (they may differ from file to file: the
files of one rate are separated together); the outputs come back at --output_rate (default: the rate of their input)."""
import os
import wave

import numpy as np

import config
from experiments.evaluation import separate as one


def build_parser():
    from utils.trainer import MyArgs
    p = MyArgs()
    p.parser.add_argument('--model_folder', help='Path to the Model folder to load', required=True)
    p.parser.add_argument('--sortofmodel', help='Sort of model', required=True)
    p.parser.add_argument('--inputs', nargs='+', help='Recordings to separate: 16-bit PCM mono .wav at %d Hz, or .npy float32 [N]; with '
                          '--resample 16-bit PCM .wav of 1 .. 8 channels at any common rate' % config.fs, required=False, default=None)
    p.parser.add_argument('--input_list', help='A text file with one input path per line (instead of --inputs)', required=False, default=None)
    p.parser.add_argument('--output_dir', help='Outputs are written to <output_dir>/<stem>_<k>.wav (.npy for an .npy input)', required=True)
    p.parser.add_argument('--hop', type=int, help='Samples between two chunks, ceil(chunk_size / 2) .. chunk_size - 1 '
                          '(default: half a chunk)', required=False, default=None)
    p.parser.add_argument('--resample', action='store_true', help='Accept other sample rates and several channels: mix down, resample '
                          'to %d Hz, separate, and resample the outputs back, all on the GPU' % config.fs)
    p.parser.add_argument('--output_rate', type=int, help='Sample rate of the outputs with --resample (default: the rate of each input)',
                          required=False, default=None)
    p.parser.add_argument('--clustering', choices=['chunk', 'recording'], default='chunk', help="k-means per chunk with the outputs tracked "
                          "across the chunk borders (default), or ONE k-means per recording over the embeddings of all its chunks "
                          "(hard k-means only; DESIGN.md 4.10)")
    p.add_adapt_args()
    p.add_separator_args()
    return p


def input_paths(args):
    """The inputs in the order given; refuses none, both sources at once, and two inputs that would write the same outputs."""
    if (args.inputs is None) == (args.input_list is None):
        raise SystemExit('give the recordings with --inputs a.wav b.wav ... or with --input_list file (one of the two)')
    if args.inputs is not None:
        paths = list(args.inputs)
    else:
        with open(args.input_list) as f:
            paths = [ln.strip() for ln in f if ln.strip()]
    if not paths:
        raise SystemExit('%s names no input' % args.input_list)
    stems = {}
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        if stem in stems:
            raise SystemExit('%s and %s would both be written to %s_<k>: give every input a file name of its own'
                             % (stems[stem], p, os.path.join(args.output_dir, stem)))
        stems[stem] = p
    return paths


def wav_rate(path):
    with wave.open(path, 'rb') as w:
        return w.getframerate()


def read_all(paths, resample):
    """[(x, rate)]: float32 [N] at config.fs, or with --resample int16 frames [N, CH] at the file's rate.  Refuses empty inputs, and
    without --resample inputs whose rates differ (before any of them is read in full)."""
    if resample:
        if any(p.endswith('.npy') for p in paths):
            raise SystemExit('--resample takes .wav inputs: an .npy array carries no sample rate')
        recs = [one.read_recording(p) for p in paths]
    else:
        rates = sorted(set(wav_rate(p) for p in paths if not p.endswith('.npy')))
        if len(rates) > 1:
            raise SystemExit('the inputs have differing sample rates (%s Hz): --resample brings every one to %d Hz on the GPU'
                             % (', '.join(str(r) for r in rates), config.fs))
        recs = [(one.read_input(p), config.fs) for p in paths]
    for p, (x, _) in zip(paths, recs):
        if x.shape[0] < 1:
            raise SystemExit('%s is empty' % p)
    return recs


def main(argv=None):
    args = build_parser().get_args(argv)
    if 'pretraining' in args.sortofmodel:
        raise SystemExit('--sortofmodel %s: a pretraining model separates with masks made from the clean sources; a recording comes '
                         'without them' % args.sortofmodel)
    if args.output_rate is not None and not args.resample:
        raise SystemExit('--output_rate goes with --resample')
    paths = input_paths(args)
    recs = read_all(paths, args.resample)
    if args.resample:
        from ams_hip import resample
        for p, (_, fs) in zip(paths, recs):
            try:
                resample.ratio(fs, config.fs)
                resample.ratio(config.fs, fs if args.output_rate is None else args.output_rate)
            except ValueError as e:
                raise SystemExit('%s: %s' % (p, e))
    from experiments.evaluation.eval import pick
    inferencer, sep = pick(args.sortofmodel)
    tr = inferencer(sep, 'inference', **vars(args))
    model = tr.prepare_inference()
    outs = [None] * len(paths)
    with tr.graph.as_default():
        if args.resample:
            for fs in sorted(set(fs for _, fs in recs)):          # the files of one rate together
                idx = [i for i, (_, f) in enumerate(recs) if f == fs]
                res = model.separate_recordings([recs[i][0] for i in idx], hop=args.hop, fs=fs, output_fs=args.output_rate,
                                                clustering=args.clustering)
                for i, o in zip(idx, res):
                    outs[i] = o.cpu().numpy()
        else:
            outs = [o.cpu().numpy() for o in model.separate_recordings([x for x, _ in recs], hop=args.hop, clustering=args.clustering)]
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    for p, (_, fs), out in zip(paths, recs, outs):
        stem = os.path.splitext(os.path.basename(p))[0]
        out_fs = (fs if args.output_rate is None else args.output_rate) if args.resample else None
        written += one.write_outputs(os.path.join(args.output_dir, stem), out, p.endswith('.npy'), out_fs)
    print('\n'.join(written))
    return written


if __name__ == '__main__':
    main()
