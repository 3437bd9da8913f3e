"""Device-resident form of the record datasets (data/dataset.py: RecordStream -> MixtureStream -> batched).

The host pipeline re-reads and re-decodes the TFRecord files on every pass and stacks and sums every mixture in numpy.  The audio of a
split does not change from pass to pass: only WHICH chunk of WHICH utterance meets which does.  So
  * ``ResidentRecords`` reads ``{split}_{M,F}.tfrecords`` once, normalises on the host (the host pipeline's expression, so the values
    are bit-equal) and uploads everything into one float32 device pool;
  * ``plan_pass`` restates the pipeline over (utterance id, chunk index, key) tuples -- the same ``_shuffle_buffer`` calls on the same
    ``RandomState`` seeds; the buffer's draws depend on counts only, so the order is the host pipeline's -- and returns a whole pass
    as two int32 tables;
  * one ``ams_mix_gather`` launch (csrc/mix.hip, ops.mix_gather) assembles a batch from the pool and a window of the tables.
``TFDataset(resident=True)`` / ``AMS_DATA_RESIDENT=1`` serves its batches this way, call for call those of the host path.

Memory: the pool is the split's audio as float32 (LibriSpeech train-clean-100 at 8 kHz: ~11.5 GB), each utterance padded to a
multiple of 4 floats; the tables take 12 bytes per source and example of a pass.
"""
import os
from itertools import product

import numpy as np

from data.dataset import _shuffle_buffer

GENDERS = ('M', 'F')


class ResidentRecords(object):
    """The utterances of one split.  Utterance ids run over the M file's records, then the F file's, in file order.
    Host side (what planning reads): ``lengths`` int64 [U], ``keys`` int64 [U], ``ids[g]`` the ids of gender g's file, ``utt_off``
    int64 [U] (multiples of 4).  Device side (``device`` given): ``pool`` float32, ``utt_off_dev`` int64.  ``device=None`` keeps the
    pool on the host instead (``host_pool``) -- planning and its tests need no GPU."""

    def __init__(self, folder, split, normalize=False, device=None):
        from data import tfrecord
        self.folder, self.split, self.normalize = folder, split, bool(normalize)
        audios, keys, self.ids = [], [], {}
        for g in GENDERS:
            path = os.path.join(folder, '%s_%s.tfrecords' % (split, g))
            if not os.path.exists(path):
                continue
            first = len(audios)
            for audio, key in tfrecord.read_audio_records(path):
                if self.normalize:                                   # RecordStream's expression, once per utterance instead of per pass
                    audio = (audio - audio.mean()) / np.sqrt(audio.var())
                audios.append(audio.astype(np.float32, copy=False))
                keys.append(key)
            self.ids[g] = list(range(first, len(audios)))
        self.lengths = np.array([a.shape[0] for a in audios], dtype=np.int64)
        self.keys = np.array(keys, dtype=np.int64)
        padded = (self.lengths + 3) // 4 * 4
        self.utt_off = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64) if len(audios) else np.zeros(0, np.int64)
        self.pool_floats = max(int(padded.sum()), 4)
        self.pool_bytes = 4 * self.pool_floats
        self.device = device
        self.host_pool = self.pool = self.utt_off_dev = None
        if device is None:
            self.host_pool = self._fill(np.zeros(self.pool_floats, dtype=np.float32), audios)
            return
        import torch
        device = torch.device(device)
        if device.type == 'cuda':
            free, total = torch.cuda.mem_get_info(device)
            if self.pool_bytes > free:
                raise MemoryError('resident %s pool under %s needs %d bytes, the device has %d free of %d: use the host pipeline '
                                  '(resident=False / AMS_DATA_RESIDENT=0)' % (split, folder, self.pool_bytes, free, total))
        self.pool = torch.empty(self.pool_floats, dtype=torch.float32, device=device)
        self.pool.copy_(torch.from_numpy(self._fill(np.zeros(self.pool_floats, dtype=np.float32), audios)))
        self.utt_off_dev = torch.from_numpy(self.utt_off if len(audios) else np.zeros(1, np.int64)).to(device)

    def _fill(self, host, audios):
        for off, a in zip(self.utt_off, audios):
            host[off:off + a.shape[0]] = a
        return host

    def validate(self, plan, L):
        """Every (utterance, chunk) of a plan [n, S, 2] lies inside its utterance: (c + 1) L <= length.  The kernel trusts the plan."""
        plan = np.asarray(plan).reshape(-1, 2).astype(np.int64)
        if plan.shape[0] == 0:
            return
        u, c = plan[:, 0], plan[:, 1]
        if u.min() < 0 or u.max() >= self.lengths.shape[0]:
            raise ValueError('plan names utterance %d of %d' % (int(u.max() if u.min() >= 0 else u.min()), self.lengths.shape[0]))
        bad = np.nonzero((c < 0) | ((c + 1) * int(L) > self.lengths[u]))[0]
        if bad.size:
            i = int(bad[0])
            raise ValueError('plan entry (utterance %d, chunk %d) at chunk size %d reaches past the utterance (%d samples)'
                             % (int(u[i]), int(c[i]), int(L), int(self.lengths[u[i]])))


def _index_stream(rec, g, L, seed):
    """RecordStream over (utterance id, chunk index, key) tuples: shuffle(100) -> keep utterances longer than the chunk (strict) ->
    floor(length / L) chunks -> shuffle(10), on RecordStream's two generators."""
    if g not in rec.ids:
        raise IOError('no %s_%s.tfrecords under %s' % (rec.split, g, rec.folder))
    rng1, rng2 = np.random.RandomState(seed), np.random.RandomState(seed + 7919)
    lengths, keys = rec.lengths, rec.keys

    def chunks():
        for u in _shuffle_buffer(iter(rec.ids[g]), 100, rng1):
            n = int(lengths[u])
            if not L < n:
                continue
            for i in range(n // L):
                yield u, i, int(keys[u])
    return _shuffle_buffer(chunks(), 10, rng2)


def _index_mixtures(streams, dropped):
    """MixtureStream: zip, drop tuples with a repeated key (counted in dropped[0])."""
    for items in zip(*streams):
        ks = [k for _, _, k in items]
        if len(set(ks)) != len(ks):
            dropped[0] += 1
            continue
        yield [(u, c) for u, c, _ in items], ks


def _round_robin(streams):
    for round_ in zip(*streams):
        for ex in round_:
            yield ex


class Plan(object):
    """One pass: ``table`` int32 [n, S, 2] = (utterance, chunk), ``keys`` int32 [n, S], ``nb_batches`` (the last one short unless
    drop_remainder), ``dropped`` = tuples the distinct-speaker filter removed."""

    def __init__(self, table, keys, batch_size, dropped, L):
        self.table, self.keys, self.batch_size, self.dropped, self.L = table, keys, int(batch_size), int(dropped), int(L)
        self.n = int(table.shape[0])
        self.nb_batches = -(-self.n // self.batch_size)
        self.table_dev = self.keys_dev = None

    def batch(self, k):
        """(first, size) of batch k."""
        first = k * self.batch_size
        return first, min(self.batch_size, self.n - first)

    def upload(self, device):
        import torch
        if self.table_dev is None and self.n:
            self.table_dev = torch.from_numpy(self.table).to(device)
            self.keys_dev = torch.from_numpy(self.keys).to(device)
        return self


def plan_pass(rec, sex, S, chunk_size, batch_size, no_random_picking=True, epoch=0, drop_remainder=False):
    """record_mixture_stream (data/dataset.py) as an index plan: the same three branches, stream seeds, epoch bump and batching."""
    S, L = int(S), int(chunk_size)
    bump = 104729 * int(epoch)
    dropped = [0]

    def stream(g, seed):
        return _index_stream(rec, g, L, seed + bump)
    both = 'M' in sex and 'F' in sex
    if both and not no_random_picking:
        combos = [_index_mixtures([stream(g, j + S * i) for j, g in enumerate(comb)], dropped)
                  for i, comb in enumerate(product(['M', 'F'], repeat=S))]
        examples = _round_robin(combos)
    elif both:
        examples = _index_mixtures([stream('M' if i % 2 == 0 else 'F', i) for i in range(S)], dropped)
    else:
        g = 'M' if 'M' in sex else 'F'
        examples = _index_mixtures([stream(g, i) for i in range(S)], dropped)
    table, keys = [], []
    for uc, ks in examples:
        table.append(uc)
        keys.append(ks)
    n = len(table)
    if drop_remainder:
        n -= n % int(batch_size)
    table = np.asarray(table[:n], dtype=np.int32).reshape(n, S, 2)
    keys = np.asarray(keys[:n], dtype=np.int32).reshape(n, S)
    rec.validate(table, L)
    return Plan(table, keys, batch_size, dropped[0], L)


class PlanBatches(object):
    """Iterator over the batches of a plan, the counterpart of iter(record_mixture_stream(...)): yields (plan, batch index)."""

    def __init__(self, plan):
        self.plan, self.k = plan, 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.k >= self.plan.nb_batches:
            raise StopIteration
        self.k += 1
        return self.plan, self.k - 1


def gather(rec, plan, k):
    """Batch k of a plan from the device pool: (mix [B, L], non_mix [B, S, L], ind [B, S] int32), one launch."""
    from ams_hip import ops
    first, size = plan.batch(k)
    plan.upload(rec.pool.device)
    return ops.mix_gather(rec.pool, rec.utt_off_dev, plan.table_dev, plan.keys_dev, first, size, plan.L)
