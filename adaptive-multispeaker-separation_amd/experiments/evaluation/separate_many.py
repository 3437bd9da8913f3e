# coding: utf-8
"""python -m experiments.evaluation.separate_many --model_folder ... --sortofmodel {STFT,front}[_enhanced]_{DPCL,L41}
       (--inputs a.wav b.wav ... | --input_list file) --output_dir D [--hop H] [--resample [--output_rate R] [--one_stream]]

Separate many recordings in one call: the chunks of all of them go through the model as one stream of full batches, and they are cut,
tracked and cross-faded by kernels whose launch count does not depend on the number of recordings (Network.separate_recordings,
ams_hip/stitch_batch.py).  Inputs as for experiments.evaluation.separate, whose .wav and .npy helpers are used here:
16-bit PCM mono .wav at config.fs, or .npy float32 [N]; --input_list names a text file with one path per line.  Output:
D/<stem>_<k>.wav (.npy for an .npy input), k = 0 .. nb_speakers - 1, where <stem> is the input's file name without its extension --
two inputs with one stem are refused.

With --resample the inputs are 16-bit PCM .wav files of 1 .. 8 channels at any common rate (they may differ from file to file: the
files of one rate are separated together); the outputs come back at --output_rate (default: the rate of their input).  With
--one_stream the files of ALL rates are separated together, in the order given: one Network.separate_recordings call with the list of
their rates, one chunk stream, one resampler launch each way.  A chunk's k-means seeds depend on its row in the
stream, so the results differ from those of the grouping by rate: the flag is opt-in.

With --reference_dir R the separated tracks are scored against the true sources R/<stem>_<k>.wav (.npy for an .npy input), each of
the input's length: ONE ragged BSS-eval call over all recordings (utils.bss_eval.bss_eval_sources_ragged) with two sets
of estimates per recording -- the mixture repeated nb_speakers times (the "no separation" line of eval.py) and the tracks as they were
written -- and D/scores.json holds the criteria per recording, their means and the mean improvement over the mixture.
--score_both_clusterings separates under both clusterings, writes the tracks of the one --clustering names and scores both as a third
set of the same call (with --clustering recording_soft, for a model with --beta_kmeans, the pair is 'chunk' and 'recording_soft':
DESIGN.md 4.13).  Scoring is at the model's rate only: --reference_dir with --resample is refused.

With --clustering recording, --speakers auto|LO:HI (and --min_score X for LO = 1) chooses every recording's number of speakers S_r
(DESIGN.md 4.11): D/<stem>_0 .. D/<stem>_{S_r - 1} are written, and D/counts.json holds every stem's count and the scores of its
candidate counts.  Under the default metric (BSS-eval: one number of tracks for references and estimates) --speakers with
--reference_dir is refused.

With --metric si_sdr (and --reference_dir) the tracks are scored by scale-invariant SDR after the best one-to-one matching of tracks
to true sources (utils.bss_eval.si_sdr_ragged): the true sources of an input are R/<stem>_0, _1, .. as far as they
exist consecutively (1 .. 6: the recording's true count, whatever --nb_speakers is), a missed speaker is an unmatched reference and a
spurious track an unmatched estimate, the mixture is the baseline of the improvement.  scores.json then carries "metric": "si_sdr",
per recording and set the pair table, the matching, si_sdr and si_sdri per reference and the missed / spurious counts, their means
and totals, and with --speakers the count accuracy and the confusion table true count -> counted -> n."""
import json
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
    p.parser.add_argument('--one_stream', action='store_true', help='With --resample: separate the files of all rates in ONE call and one '
                          'chunk stream, in the order given, instead of one call per distinct rate (DESIGN.md 4.12)')
    p.parser.add_argument('--clustering', choices=['chunk', 'recording', 'recording_soft'], default='chunk', help="k-means per chunk with "
                          "the outputs tracked across the chunk borders (default), or ONE k-means per recording over the embeddings of all "
                          "its chunks: 'recording' for a hard k-means (DESIGN.md 4.10), 'recording_soft' for a model with --beta_kmeans "
                          "(DESIGN.md 4.13)")
    p.parser.add_argument('--reference_dir', help='Score the separated tracks against the true sources <reference_dir>/<stem>_<k>.wav '
                          '(.npy for an .npy input) and write <output_dir>/scores.json (DESIGN.md 6c)', required=False, default=None)
    p.parser.add_argument('--score_both_clusterings', action='store_true', help="With --reference_dir: separate under 'chunk' and "
                          "under 'recording' ('recording_soft' where --clustering names it), write the tracks of the one --clustering "
                          "names, score both in the same call")
    p.parser.add_argument('--metric', choices=['bss_eval', 'si_sdr'], default='bss_eval', help="With --reference_dir: 'bss_eval' (default: "
                          "SDR / SIR / SAR, one number of tracks for all) or 'si_sdr': scale-invariant SDR after the best matching of "
                          "tracks to true sources, for recordings whose numbers of tracks and of true sources differ (DESIGN.md 6d)")
    one.add_speakers_args(p.parser)
    p.add_adapt_args()
    p.add_separator_args()
    return p


def read_references(paths, recs, reference_dir, nsrc):
    """[float32 [S, N]] per input: <reference_dir>/<stem>_<k>, k = 0 .. S - 1, each of the input's length; anything else is refused with
    the file named."""
    refs = []
    for p, (x, _) in zip(paths, recs):
        stem, ext = os.path.splitext(os.path.basename(p))
        rows = []
        for k in range(nsrc):
            rp = os.path.join(reference_dir, '%s_%d%s' % (stem, k, '.npy' if ext == '.npy' else '.wav'))
            if not os.path.isfile(rp):
                raise SystemExit('%s: the true source %d of %s is missing' % (rp, k, p))
            r = one.read_input(rp)
            if r.shape[0] != x.shape[0]:
                raise SystemExit('%s has %d samples, %s has %d: a true source has the length of its mixture' % (rp, r.shape[0], p, x.shape[0]))
            rows.append(r)
        refs.append(np.stack(rows))
    return refs


def read_references_counted(paths, recs, reference_dir, most=6):
    """[float32 [S_r, N]] per input: <reference_dir>/<stem>_0, _1, .. as far as they exist consecutively -- the recording's true count,
    1 .. `most`; each of the input's length; anything else is refused with the file named."""
    refs = []
    for p, (x, _) in zip(paths, recs):
        stem, ext = os.path.splitext(os.path.basename(p))
        name = lambda k: os.path.join(reference_dir, '%s_%d%s' % (stem, k, '.npy' if ext == '.npy' else '.wav'))      # noqa: E731
        n = 0
        while os.path.isfile(name(n)):
            n += 1
        if n < 1:
            raise SystemExit('%s: the true source 0 of %s is missing' % (name(0), p))
        if n > most:
            raise SystemExit('%s: %s has more than %d true sources' % (name(most), p, most))
        rows = []
        for k in range(n):
            r = one.read_input(name(k))
            if r.shape[0] != x.shape[0]:
                raise SystemExit('%s has %d samples, %s has %d: a true source has the length of its mixture' % (name(k), r.shape[0], p, x.shape[0]))
            rows.append(r)
        refs.append(np.stack(rows))
    return refs


def score_si_sdr(paths, recs, refs, sets, counted=None):
    """sets: [(name, [tracks [S_r, N] per recording])] -> the dictionary of scores.json under --metric si_sdr.  ONE ragged call: the
    mixture is the baseline, every set a set.  counted: with --speakers the count of every recording."""
    from utils.bss_eval import si_sdr_ragged
    names = [n for n, _ in sets]
    ests = [[np.ascontiguousarray(t[i], np.float32) for _, t in sets] for i in range(len(paths))]
    out = si_sdr_ragged(refs, ests, [np.asarray(x, np.float32) for x, _ in recs])
    num = lambda v: [None if not np.isfinite(a) else float(a) for a in v]       # noqa: E731
    per = []
    pooled = {n: ([], []) for n in names}
    for i, p in enumerate(paths):
        Sr = int(refs[i].shape[0])
        entry = {'input': p, 'samples': int(refs[i].shape[1]), 'references': Sr, 'info': int(out['info'][i]), 'base': num(out['base'][i, :Sr]),
                 'sets': {}}
        for k, name in enumerate(names):
            Se = int(ests[i][k].shape[0])
            entry['sets'][name] = {'tracks': Se, 'pair': [num(row[:Sr]) for row in out['pair'][i, k, :Se]],
                                   'match_ref': [int(v) for v in out['match_ref'][i, k, :Sr]],
                                   'match_est': [int(v) for v in out['match_est'][i, k, :Se]],
                                   'si_sdr': num(out['si_sdr'][i, k, :Sr]), 'si_sdri': num(out['si_sdri'][i, k, :Sr]),
                                   'missed': int(out['missed'][i, k]), 'spurious': int(out['spurious'][i, k])}
            if out['info'][i] == 0:
                m = out['match_ref'][i, k, :Sr] >= 0
                pooled[name][0].extend(out['si_sdr'][i, k, :Sr][m].tolist())
                pooled[name][1].extend(out['si_sdri'][i, k, :Sr][m].tolist())
        per.append(entry)
    good = out['info'] == 0
    mean = lambda v: num([np.mean(v)])[0] if len(v) else None                   # noqa: E731
    res = {'metric': 'si_sdr', 'zero_mean': True, 'sets': names, 'recordings': per, 'scored': int(good.sum()),
           'means': {n: {'si_sdr': mean(pooled[n][0]), 'si_sdri': mean(pooled[n][1])} for n in names},
           'missed': {n: int(out['missed'][good, k].sum()) for k, n in enumerate(names)},
           'spurious': {n: int(out['spurious'][good, k].sum()) for k, n in enumerate(names)}}
    if counted is not None:
        true = [int(r.shape[0]) for r in refs]
        res['count_accuracy'] = float(np.mean([c == t for c, t in zip(counted, true)]))
        table = {}
        for c, t in zip(counted, true):
            row = table.setdefault(str(t), {})
            row[str(int(c))] = row.get(str(int(c)), 0) + 1
        res['confusion'] = table
    return res


def as_written(out, as_npy):
    """The tracks as write_outputs stores them and read_input reads them back: float32, through 16-bit PCM for a .wav."""
    out = np.asarray(out)
    if as_npy:
        return np.asarray(out, np.float32)
    if not np.all(np.isfinite(out)):
        raise SystemExit('%d of %d separated samples are not finite; nothing scored' % (int((~np.isfinite(out)).sum()), out.size))
    pcm = np.clip(np.rint(np.asarray(out, np.float64) * 32768.0), -32767, 32767).astype('<i2')
    return pcm.astype(np.float32) / np.float32(32768.0)


def score(paths, recs, refs, sets):
    """sets: [(name, [tracks [S, N] per recording])] -> the dictionary of scores.json.  ONE ragged call: per recording the mixture
    repeated S times, then every set."""
    from utils.bss_eval import bss_eval_pairs_ragged, _select_permutation
    S = refs[0].shape[0]
    names = ['mixture'] + [n for n, _ in sets]
    ests = []
    for i, (x, _) in enumerate(recs):
        ests.append(np.stack([np.repeat(np.asarray(x, np.float32)[None], S, axis=0)] + [t[i] for _, t in sets]))
    crit, info = bss_eval_pairs_ragged(refs, ests)
    num = lambda v: [None if not np.isfinite(a) else float(a) for a in v]       # noqa: E731
    per, good = [], []
    for i, p in enumerate(paths):
        entry = {'input': p, 'samples': int(refs[i].shape[1]), 'info': int(info[i]), 'sets': {}}
        vals = np.empty((len(names), 3, S))
        for k, name in enumerate(names):
            sdr, sir, sar, perm = _select_permutation(crit[i, k, 0], crit[i, k, 1], crit[i, k, 2])
            vals[k] = sdr, sir, sar
            entry['sets'][name] = {'sdr': num(sdr), 'sir': num(sir), 'sar': num(sar), 'perm': [int(v) for v in perm]}
        per.append(entry)
        if info[i] == 0:
            good.append(vals)
    res = {'flen': 512, 'sets': names, 'recordings': per, 'scored': len(good), 'means': None, 'improvement': None}
    if good:
        m = np.mean(np.stack(good), axis=(0, 3))                               # [set, criterion]
        crits = ('sdr', 'sir', 'sar')
        res['means'] = {n: {c: float(m[k, j]) for j, c in enumerate(crits)} for k, n in enumerate(names)}
        res['improvement'] = {n: {c: float(m[k, j] - m[0, j]) for j, c in enumerate(crits)} for k, n in enumerate(names) if k}
    return res


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
    if args.one_stream and not args.resample:
        raise SystemExit('--one_stream goes with --resample')
    if args.score_both_clusterings and args.reference_dir is None:
        raise SystemExit('--score_both_clusterings goes with --reference_dir')
    if args.reference_dir is not None and args.resample:
        raise SystemExit('--reference_dir with --resample: scoring at a rate other than the model\'s %d Hz is not built' % config.fs)
    if args.metric == 'si_sdr' and args.reference_dir is None:
        raise SystemExit('--metric si_sdr goes with --reference_dir')
    if args.speakers is not None and args.reference_dir is not None and args.metric != 'si_sdr':
        raise SystemExit('--speakers with --reference_dir: scoring recordings of differing numbers of tracks by BSS-eval is not built; '
                         '--metric si_sdr scores them')
    if args.speakers is not None and args.score_both_clusterings:
        raise SystemExit('--speakers with --score_both_clusterings: counting under both clusterings is not built')
    speakers = one.speakers_arg(args)
    seeding = one.seeding_arg(args, whole=args.score_both_clusterings)
    paths = input_paths(args)
    recs = read_all(paths, args.resample)
    if args.reference_dir is None:
        refs = None
    elif args.metric == 'si_sdr':
        refs = read_references_counted(paths, recs, args.reference_dir)
    else:
        refs = read_references(paths, recs, args.reference_dir, args.nb_speakers)
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
    other = None
    counted = [None] * len(paths)                                 # with --speakers: (count, scores of the candidate counts) per input
    spk = dict(speakers=speakers, min_score=args.min_score, recording_seeding=seeding)

    def note(idx):
        if speakers is not None:
            lc = model.last_clustering
            for i, c, sc in zip(idx, lc['counts'].tolist(), lc['scores'].tolist()):
                counted[i] = (int(c), sc)
    with tr.graph.as_default():
        if args.score_both_clusterings:
            # a soft k-means model is refused here, with the message clustering='recording' gives, before anything is separated; the
            # clustering whose tracks are written runs first, so that it draws the k-means seeds it draws without scoring
            # (--clustering recording_soft: the pair is 'chunk' and 'recording_soft', and a hard model is refused the same way)
            whole = 'recording_soft' if args.clustering == 'recording_soft' else 'recording'
            model._check_clustering(whole, None, len(recs))
            mode = whole if args.clustering == 'chunk' else 'chunk'
            xs = [x for x, _ in recs]
            # (--recording_seeding goes to the clustering of whole recordings of the pair; 'chunk' has no such seeds)
            how = lambda m: {} if m == 'chunk' else {'recording_seeding': seeding}          # noqa: E731
            outs = [o.cpu().numpy() for o in model.separate_recordings(xs, hop=args.hop, clustering=args.clustering, **how(args.clustering))]
            other = (mode, [o.cpu().numpy() for o in model.separate_recordings(xs, hop=args.hop, clustering=mode, **how(mode))])
        elif args.resample and args.one_stream:
            res = model.separate_recordings([x for x, _ in recs], hop=args.hop, fs=[fs for _, fs in recs], output_fs=args.output_rate,
                                            clustering=args.clustering, **spk)
            note(range(len(paths)))
            outs = [o.cpu().numpy() for o in res]
        elif args.resample:
            for fs in sorted(set(fs for _, fs in recs)):          # the files of one rate together
                idx = [i for i, (_, f) in enumerate(recs) if f == fs]
                res = model.separate_recordings([recs[i][0] for i in idx], hop=args.hop, fs=fs, output_fs=args.output_rate,
                                                clustering=args.clustering, **spk)
                note(idx)
                for i, o in zip(idx, res):
                    outs[i] = o.cpu().numpy()
        else:
            outs = [o.cpu().numpy() for o in model.separate_recordings([x for x, _ in recs], hop=args.hop, clustering=args.clustering,
                                                                       **spk)]
            note(range(len(paths)))
    os.makedirs(args.output_dir, exist_ok=True)
    written = []
    for p, (_, fs), out in zip(paths, recs, outs):
        stem = os.path.splitext(os.path.basename(p))[0]
        out_fs = (fs if args.output_rate is None else args.output_rate) if args.resample else None
        written += one.write_outputs(os.path.join(args.output_dir, stem), out, p.endswith('.npy'), out_fs)
    if speakers is not None:
        lo, hi = speakers
        num = lambda v: None if not np.isfinite(v) else float(v)               # noqa: E731  (a disqualified candidate: -inf -> null)
        cj = {'speakers': [lo, hi], 'min_score': args.min_score, 'candidates': list(range(max(lo, 2), hi + 1)), 'recordings': {}}
        for p, (c, sc) in zip(paths, counted):
            cj['recordings'][os.path.splitext(os.path.basename(p))[0]] = {'count': c, 'scores': [num(v) for v in sc]}
        cp = os.path.join(args.output_dir, 'counts.json')
        with open(cp, 'w') as f:
            json.dump(cj, f, indent=1)
        written.append(cp)
    if refs is not None:
        npy = [p.endswith('.npy') for p in paths]
        sets = [(args.clustering if other else 'separated', [as_written(o, n) for o, n in zip(outs, npy)])]
        if other:
            sets.append((other[0], [as_written(o, n) for o, n in zip(other[1], npy)]))
            sets.sort(key=lambda s: ('chunk', 'recording', 'recording_soft').index(s[0]))
        if args.metric == 'si_sdr':
            scores = score_si_sdr(paths, recs, refs, sets, None if speakers is None else [c for c, _ in counted])
        else:
            scores = score(paths, recs, refs, sets)
        sp = os.path.join(args.output_dir, 'scores.json')
        with open(sp, 'w') as f:
            json.dump(scores, f, indent=1)
        written.append(sp)
    print('\n'.join(written))
    return written


if __name__ == '__main__':
    main()
