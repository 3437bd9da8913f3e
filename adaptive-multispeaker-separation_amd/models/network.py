# -*- coding: utf-8 -*-
"""Host mirror of the reference's model-construction API (reference models/network.py).

Same classes, constructor kwargs, lazily-built attribute names and session-facing methods -- ``Network`` and
``Separator`` -- so ``utils/trainer.py`` recipes read like the reference's.  Attributes that were TF tensors are
``ams_hip.graph.Node`` objects evaluated once per ``train/valid_batch/...`` call; their bodies launch the HIP
kernels of libams_hip.so (no TF, no CPU fallback).
"""
import json
import os
import random

import numpy as np
import torch

import config
from ams_hip import functional as F
from ams_hip import ops as K
from ams_hip.graph import Node, Placeholder, Run, get_default_graph, scope
from ams_hip.optim import FlatOptimizer
from utils.ops import BLSTM, Conv1D, Conv2D, conv2d_stack, f_props

_ADJ = ['autumn', 'hidden', 'bitter', 'misty', 'silent', 'empty', 'dry', 'dark', 'summer', 'icy', 'quiet', 'white', 'cool',
        'spring', 'winter', 'patient', 'twilight', 'dawn', 'crimson', 'wispy', 'weathered', 'blue', 'billowing', 'broken']
_NOUN = ['waterfall', 'river', 'breeze', 'moon', 'rain', 'wind', 'sea', 'morning', 'snow', 'lake', 'sunset', 'pine', 'shadow',
         'leaf', 'dawn', 'glitter', 'forest', 'hill', 'cloud', 'meadow', 'sun', 'glade', 'bird', 'brook']


def haikunate():
    """Stand-in for haikunator.Haikunator().haikunate() (network.py:35): adjective-noun-4digits."""
    r = random.SystemRandom()
    return '%s-%s-%04d' % (r.choice(_ADJ), r.choice(_NOUN), r.randint(0, 9999))


class SummaryWriter(object):
    """JSON-lines stand-in for tf.summary.FileWriter (network.py:120-122); off the timed path."""

    def __init__(self, path):
        self.path = path
        self._f = None

    def add(self, step, values):
        if self._f is None:
            os.makedirs(self.path, exist_ok=True)
            self._f = open(os.path.join(self.path, 'events.jsonl'), 'a')
        self._f.write(json.dumps({'step': int(step), 'values': values}) + '\n')
        self._f.flush()


class Network(object):
    """docstring for Network"""

    def __init__(self, graph=None, *args, **kwargs):
        # Constant seed for uniform results (network.py:17-18)
        np.random.seed(42)

        if kwargs is not None and len(kwargs):
            self.folder = kwargs['type']
            self.S = kwargs['nb_speakers']
            if self.S > 6:
                # six is what can be scored and searched: both BSS-eval libraries take nsrc <= 6 (csrc/bss), and the permutation search
                # of the PIT costs (csrc/synth.hip pair_search_kernel) covers the 720 permutations of six speakers; say so at
                # construction, not as AMS_E_INVALID_ARG in a step
                raise ValueError('--nb_speakers %d: at most 6 speakers -- the limit of BSS-eval scoring (nsrc <= 6) and of the '
                                 'permutation search of the PIT costs (6! = 720 permutations)' % self.S)
            self.args = kwargs
            self.learning_rate = kwargs['learning_rate']
            self.my_opt = kwargs['optimizer']
            self.decay_epoch = kwargs['decay_epoch']
            self.gradient_clip = kwargs['gradient_norm_clip']
        else:
            raise Exception('Keyword Arguments missing ! Please add the right arguments in input | check doc')

        self.dist = kwargs.get('dist', None)
        self.summaries_enabled = kwargs.get('summaries', True)

        if graph is None:
            # Run ID
            # one run folder for the whole job: with N ranks the id is chosen on rank 0 and broadcast (save() writes on rank 0
            # only, every rank restores from that folder at the end of Trainer.train)
            self.runID = kwargs.get('run_id') or haikunate()
            if self.dist is not None and getattr(self.dist, 'enabled', False) and not kwargs.get('run_id'):
                self.runID = self.dist.broadcast_object(self.runID)
            print('ID : {}'.format(self.runID))
            g = get_default_graph()
            with g.variable_scope('inputs'):
                self.training = Placeholder('is_training')
                if not kwargs['pipeline']:
                    # fed through feed_dict (network.py:44-63)
                    self.x_non_mix = Placeholder('non_mix_input')      # [B, S, L]
                    self.x_mix = Placeholder('mix_input')              # [B, L]
                    self.I = Placeholder('indicies')                   # [B, S]
                else:
                    # tensors produced by the input pipeline (network.py:65-85)
                    nm, mx, ind = kwargs['non_mix'], kwargs['mix'], kwargs['ind']
                    self.x_non_mix = Node('non_mix_input', lambda run: nm.value(run))
                    self.x_mix = Node('mix_input', lambda run: mx.value(run))
                    self.I = Node('indicies', lambda run: ind.value(run))

    # --------------------------------------------------------------- bookkeeping
    def _dir(self):
        return os.path.join(config.log_dir, self.folder, self.runID)

    def tensorboard_init(self):
        self.create_saver()
        g = get_default_graph()
        train_keys, valid_keys, test_keys = [], [], []
        for name in g.summaries:                                        # network.py:98-107
            if not ('input' in name or 'output' in name):
                train_keys.append(name)
            else:
                valid_keys.append(name)
            if 'SDR_improvement' in name:
                valid_keys.append(name)
                test_keys.append(name)
            if 'audio' in name or 'stft' in name or 'mask' in name:
                test_keys.append(name)
        self.merged_train = train_keys
        self.merged_valid = valid_keys if len(valid_keys) else None
        self.merged_test = test_keys if len(test_keys) else None
        self.train_writer = SummaryWriter(os.path.join(self._dir(), 'train'))
        self.valid_writer = SummaryWriter(os.path.join(self._dir(), 'valid'))
        self.test_writer = SummaryWriter(os.path.join(self._dir(), 'test'))
        # Save arguments (network.py:124-129)
        if self.dist is None or self.dist.rank == 0:
            os.makedirs(self._dir(), exist_ok=True)
            with open(os.path.join(self._dir(), 'params'), 'w') as f:
                for k in ('mix', 'non_mix', 'ind'):
                    self.args.pop(k, None)
                json.dump({k: v for k, v in self.args.items() if _jsonable(v)}, f)

    def create_saver(self, subset=None):
        g = get_default_graph()
        self.saver = list(g.variables.keys()) if subset is None else [v.ams_name for v in subset]

    def _latest_checkpoint(self, path):
        marker = os.path.join(path, 'checkpoint')
        if os.path.exists(marker):
            with open(marker) as f:
                name = json.load(f)['model_checkpoint_path']
            return os.path.join(path, name)
        cands = sorted([p for p in os.listdir(path) if p.startswith('model-') and p.endswith('.npz')],
                       key=lambda p: int(p[6:-4]))
        if not cands:
            raise IOError('no checkpoint in %s' % path)
        return os.path.join(path, cands[-1])

    # Restore last checkpoint of the current graph using the total path (network.py:139-140)
    def restore_model(self, path):
        g = get_default_graph()
        # a folder written by the REFERENCE (tf.train.Saver: text `checkpoint` file + model-N.index/.data-*) is read directly
        from ams_hip import tf_checkpoint
        marker = os.path.join(path, 'checkpoint')
        is_tf = os.path.exists(marker) and open(marker).read(22).startswith('model_checkpoint_path')
        if is_tf:
            prefix = tf_checkpoint.latest_checkpoint(path)
            bundle = tf_checkpoint.read_bundle(prefix, names=set(self.saver))
            for name in self.saver:
                if name not in bundle:
                    # the BLSTM / dense / speaker-vector names are inferred from the reference's scopes, never
                    # observed in a TensorFlow-written file: say what the bundle does hold, so a renamed variable is one edit away
                    have = sorted(tf_checkpoint.list_bundle(prefix)[1])
                    raise KeyError('variable %s not found in TensorFlow checkpoint %s; the bundle holds: %s' % (name, prefix, ', '.join(have)))
                v = g.variables[name]
                arr = bundle[name]
                if tuple(arr.shape) != tuple(v.shape):
                    # the reference's Conv1D kernels are 3-D [1, Din, Dout] (utils/ops.py:486-492); here they are [Din, Dout]
                    squeezed = tuple(d for d in arr.shape if d != 1)
                    if squeezed != tuple(d for d in v.shape if d != 1):
                        raise ValueError('variable %s: checkpoint shape %s, graph shape %s' % (name, arr.shape, tuple(v.shape)))
                    arr = arr.reshape(tuple(v.shape))
                v.data.copy_(torch.from_numpy(arr.astype(np.float32)).to(v.device))
                g.initialized.add(name)
            self._weights_written()
            return
        data = np.load(self._latest_checkpoint(path))
        for name in self.saver:
            key = name.replace('/', '.')
            if key not in data.files:
                raise KeyError('variable %s not found in checkpoint %s' % (name, path))
            v = g.variables[name]
            v.data.copy_(torch.from_numpy(data[key]).to(v.device))
            g.initialized.add(name)
        self._weights_written()

    @staticmethod
    def _weights_written():
        """Variables were written by something other than an optimizer kernel: what captured steps keep across replays instead of
        re-deriving it from the weights (the weights' operand bound, a frozen front's filter) must be refreshed."""
        g = get_default_graph()
        g.weights_epoch = getattr(g, 'weights_epoch', 0) + 1
        if torch.cuda.is_available():
            K.param_bounds_dirty()
        for v in g.variables.values():                 # (freeze_weights: what was derived from the old values)
            K.drop_frozen_derivatives(v)

    def freeze_weights(self):
        """Inference recipes (no optimizer is ever built): nothing writes the variables between passes, so what a pass derives from
        them alone -- operand bounds of the fp16x3 products, the gathered [D, 8H] projection kernels, concatenated biases -- is kept
        across passes (ams_hip/ops.py::_frozen) instead of being re-derived in each: ~45 us of launches per BLSTM layer and pass in
        an eager inference step, and the recurrent product of the rings gets a bound, i.e. runs as fp16x3 as in training.
        restore_model() / anything that calls _weights_written() drops the derived tensors; code that writes `.data` of a variable
        behind the model's back must call _weights_written() itself (as it must for captured steps)."""
        for v in get_default_graph().variables.values():
            K.set_frozen(v, True)

    def restore_last_checkpoint(self):
        self.restore_model(self._dir())

    def init_all(self):
        g = get_default_graph()
        g.initialized.update(g.variables.keys())      # variables are materialised with their initial value

    def non_initialized_variables(self):
        g = get_default_graph()
        return [n for n in g.variables if n not in g.initialized]

    def initialize_non_init(self):
        names = self.non_initialized_variables()
        print('not init: ', names)
        get_default_graph().initialized.update(names)

    @scope
    def optimize(self):
        print('Train the following variables :', [v.ams_name for v in self.trainable_variables])
        g = get_default_graph()
        for v in g.global_variables():
            v.requires_grad_(False)
        for v in self.trainable_variables:             # (an earlier freeze_weights() / optimize(): the optimizer writes these from now on)
            K.set_frozen(v, False)
        opt = FlatOptimizer(self.trainable_variables, self.my_opt, self.learning_rate, self.decay_epoch,
                            self.gradient_clip, self.dist)
        F.OVERLAP.enabled = (bool(self.args.get('overlap_weight_grads', True)) and torch.cuda.is_available()
                             and os.environ.get('AMS_OVERLAP', '1') != '0')
        F.OVERLAP.on_ready = opt.bucket_ready if getattr(opt, 'overlap', False) else None
        # Variables this recipe does NOT train (a restored separator under an enhance stack, a restored front end) are written by nobody
        # between passes -- the optimizer owns only the trainable ones, and restore_model() / _weights_written() drop what was derived:
        # what a pass derives from them alone (operand bounds, pre-split images, gathered kernels) is kept across passes as in the
        # inference recipes (freeze_weights): 13 absmax + fill pairs and 4 image cuts per STFT_L41_enhance step otherwise
        if os.environ.get('AMS_FREEZE_UNTRAINED', '1') != '0':
            trained = set(id(v) for v in self.trainable_variables)
            for v in g.variables.values():
                if id(v) not in trained:
                    K.set_frozen(v, True)
        self.optimizer = opt
        self.increment_epoch = opt.increment_epoch
        g.summaries['optimize/learning_rate'] = Node('learning_rate', lambda run: opt.learning_rate())
        return opt

    def sdr_improvement(self, s_target, s_approx, with_perm=False):
        """network.py:196-221 -- built by models that own a waveform output (Adapt.back, postprocessing)."""
        from ams_hip import losses_host
        return losses_host.sdr_improvement(self, s_target, s_approx, with_perm)

    # --------------------------------------------------------------- checkpoints
    def save(self, step):
        path = os.path.join(self._dir(), 'model')
        if self.dist is None or self.dist.rank == 0:
            g = get_default_graph()
            os.makedirs(self._dir(), exist_ok=True)
            arrays = {n.replace('/', '.'): g.variables[n].detach().cpu().numpy() for n in self.saver}
            fname = 'model-%d.npz' % step
            np.savez(os.path.join(self._dir(), fname), **arrays)
            with open(os.path.join(self._dir(), 'checkpoint'), 'w') as f:
                json.dump({'model_checkpoint_path': fname}, f)
        return path

    # --------------------------------------------------------------- session-facing methods
    def _feeds(self, feed_dict, training, new_pass=True):
        feeds = dict(feed_dict)
        feeds[self.training] = training
        return Run(feeds, training, new_pass)

    def _summaries(self, run, keys):
        g = get_default_graph()
        out = {}
        for k in keys or []:
            v = g.summaries[k].value(run)
            out[k] = float(v) if not torch.is_tensor(v) else float(v.detach().reshape(-1)[0].item())
        return out

    # ---- hipGraph replay of forward+backward (the launch-bound inner loops: 80 recurrent steps x 6 cells x 2) ----
    def _fetch_inputs(self, feed_dict):
        """One batch from the input pipeline (a probe Run that only evaluates the input nodes)."""
        # the probe only fetches the input nodes: it must NOT begin a pass (ops.pass_begin clears the ring arena and rewrites the shared
        # weight bound on the side stream, un-joined, while the replayed graph owns both addresses) nor count as one
        probe = self._feeds(feed_dict, True, new_pass=False)
        return [n.value(probe) for n in (self.x_mix, self.x_non_mix, self.I)]

    @staticmethod
    def _back_to_back(a, b):
        return (a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype and a.device == b.device and
                a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr() and
                a.data_ptr() + a.numel() * a.element_size() == b.data_ptr())

    @staticmethod
    def _static_like(ins):
        """Static input buffers of a captured step: x_mix [B,L] and x_non_mix [B,S,L] back to back in one buffer (Adapt's
        concat([x_mix, x_non_mix rows]) is then a view), the rest cloned."""
        xm, xn = ins[0], ins[1]
        if xm.dtype == xn.dtype and xm.dim() == 2 and xn.dim() == 3 and xm.shape[-1] == xn.shape[-1]:
            flat = torch.empty(xm.numel() + xn.numel(), dtype=xm.dtype, device=xm.device)
            sm, sn = flat[:xm.numel()].view(xm.shape), flat[xm.numel():].view(xn.shape)
            sm.copy_(xm)
            sn.copy_(xn)
            return [sm, sn] + [t.clone() for t in ins[2:]]
        return [t.clone() for t in ins]

    def _stage(self, static, ins):
        """This batch into the static buffers of the captured step.  x_mix and x_non_mix adjacent on both sides (_static_like; the
        synthetic pool stores them so): ONE launch moves them, the small third input (speaker indices) with them, and leaves
        max |waveform| -- the front product's operand bound -- on the way (K.stage_inputs); anything else: plain copies."""
        pairs = list(zip(static, ins))
        if (self._back_to_back(static[0], static[1]) and self._back_to_back(ins[0], ins[1]) and ins[0].is_cuda
                and ins[0].dtype == torch.float32 and ins[0].data_ptr() % 16 == 0 and static[0].data_ptr() % 16 == 0):
            n = ins[0].numel() + ins[1].numel()
            src2 = dst2 = None
            rest = pairs[2:]
            if len(rest) == 1 and rest[0][1].is_contiguous() and rest[0][0].is_contiguous() and rest[0][1].numel() * rest[0][1].element_size() <= 65536:
                dst2, src2 = rest[0]
                rest = []
            am = K.stage_inputs(torch.as_strided(ins[0], (n,), (1,)), torch.as_strided(static[0], (n,), (1,)), src2, dst2)
            static[0]._ams_x_amax = am              # models/adapt.py::Adapt._x tags the concatenated view with it
            pairs = rest
            for dst, src in pairs:
                dst.copy_(src)
            return
        for dst, src in pairs:
            dst.copy_(src)
        am = getattr(static[0], '_ams_x_amax', None)
        if am is not None and static[0].is_cuda:
            # an earlier batch went through the fused launch and the captured step holds the address of its bound: this batch came by
            # plain copies (not back to back / not aligned), so the bound is measured over what was just copied -- never left stale
            # (a louder batch under a stale max |x| overflows fp16 in the front product: ADVICE r05)
            flat = static[0]
            if self._back_to_back(static[0], static[1]):
                flat = torch.as_strided(static[0], (static[0].numel() + static[1].numel(),), (1,))
                K.absmax(flat, out=am)
            else:
                K.absmax(static[0].reshape(-1), out=am)
                K.absmax(static[1].reshape(-1), out=(tmp := torch.empty_like(am)))
                torch.maximum(am, tmp, out=am)

    def _train_graphed(self, feed_dict, step):
        """Capture zero_grad + forward + backward once (after 2 eager steps) and replay it; inputs are copied into
        static buffers, the optimizer (per-step lr_t, all-reduce) stays outside the graph.
        (Round 4 built a two-graph form that computed a FROZEN front end one batch ahead, beside the previous step's forward rings:
        measured 0 ... -0.5 %, not kept -- profiles/r04_d_front_ahead_ab.txt, commits 43a78ea..dc02139.)"""
        st = self.__dict__.setdefault('_cg_state', {'n': 0, 'graph': None,
                                                    'stream': torch.cuda.Stream(priority=int(os.environ.get('AMS_MAIN_PRIORITY', '0')))})
        ins = self._fetch_inputs(feed_dict)
        opt = self.optimize
        side = st['stream']
        epoch = getattr(get_default_graph(), 'weights_epoch', 0)
        if st['graph'] is not None and st.get('epoch') != epoch:
            # somebody other than the optimizer kernel wrote weights since the capture (restore_model): what the captured step took as
            # constants -- a frozen front's filter and its bound (models/adapt.py) -- is stale.  Capture again behind two eager
            # steps, which re-derive them.
            st['graph'], st['n'] = None, 0
        if st['graph'] is None:
            st['n'] += 1
            if st['n'] <= 2:
                # eager warm-up ON THE CAPTURE STREAM, so autograd's AccumulateGrad nodes are bound to it
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    run = self._feeds(feed_dict, True)
                    for node, t in zip((self.x_mix, self.x_non_mix, self.I), ins):
                        run.cache[id(node)] = t
                    opt.zero_grad(defer=True)
                    cost = self.cost_model.value(run)
                    self._backward(cost)
                    F.OVERLAP.join()
                torch.cuda.current_stream().wait_stream(side)
                opt.step()
                self.last_run = run
                return cost.detach().reshape(-1)[0]
            st['static'] = self._static_like(ins)
            self._stage(st['static'], ins)          # (also attaches the waveforms' bound to the static buffer before the capture reads it)

            def capture(presplit):
                run = self._feeds(feed_dict, True)
                for node, t in zip((self.x_mix, self.x_non_mix, self.I), st['static']):
                    run.cache[id(node)] = t
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                # thread_local: a collective library's watchdog thread (RCCL at N > 1) must not be able to invalidate this capture
                with K.presplit(presplit), torch.cuda.graph(g, stream=side, capture_error_mode='thread_local'):
                    opt.zero_grad(defer=True)
                    cost = self.cost_model.value(run)
                    self._backward(cost)
                    F.OVERLAP.join()
                return g, cost, run
            # Which form of the forward products this step replays (K.PS_AUTOTUNE): decided once per model by measurement, see below
            choice = self.__dict__.get('_ps_choice')
            n0 = K.PS_LAUNCHES[0]
            first = K.PRESPLIT if choice is None else (choice and K.PRESPLIT)
            st['graph'], st['cost'], st['run'] = capture(first)
            st['epoch'], st['tune'] = epoch, None
            st['twin'] = capture if (K.PS_AUTOTUNE and (K.PS_LAUNCHES[0] > n0 or choice is not None)) else None      # (closes over this capture's static buffers)
            if choice is None and K.PS_AUTOTUNE and first and K.PS_LAUNCHES[0] > n0:
                # the captured step holds pre-split products: capture its twin without them and let the next steps decide.  Both are
                # the same arithmetic to the last bits (tests/test_gpu_gemm_ps.py); every tuning step is a real training step.
                st['tune'] = {'variants': [(st['graph'], st['cost'], st['run']), capture(False)], 'k': 0, 'ev': ([], [])}
        tune = st.get('tune')
        if (tune is None and self._PS_RETUNE_EVERY > 0 and K.PS_AUTOTUNE and self.__dict__.get('_ps_choice') is not None
                and st.get('since_tune', 0) >= self._PS_RETUNE_EVERY and st.get('twin') is not None):
            # a long run asks the question again (what a board's governor allows moves with its temperature): the form that lost is
            # captured anew and the two are measured as at the start
            keep = (st['graph'], st['cost'], st['run'])
            other = st['twin'](not self._ps_choice)
            st['tune'] = tune = {'variants': [keep, other] if self._ps_choice else [other, keep], 'k': 0, 'ev': ([], [])}
        st['since_tune'] = 0 if tune is not None else st.get('since_tune', 0) + 1
        if tune is not None:
            v = (tune['k'] // self._PS_TUNE_BLOCK) % 2
            st['graph'], st['cost'], st['run'] = tune['variants'][v]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        self._stage(st['static'], ins)
        for hook in get_default_graph().pre_replay_hooks:      # host-drawn inputs of captured kernels (k-means seeds)
            hook()
        st['graph'].replay()
        opt.step()
        self.last_run = st['run']
        cost = st['cost'].detach().reshape(-1)[0]
        if tune is not None:
            e1.record()
            tune['ev'][v].append((tune['k'] % self._PS_TUNE_BLOCK, e0, e1))
            tune['k'] += 1
            if tune['k'] >= 4 * self._PS_TUNE_BLOCK:
                self._ps_finish_tuning(st)
        return cost

    # steps per block; blocks alternate pre-split / in-product twice; only the last third of a block is counted: the clock governor takes
    # tens of milliseconds to settle after the form changes (blocks of 8 steps measured both forms at the slower form's clock)
    _PS_TUNE_BLOCK = int(os.environ.get('AMS_PS_TUNE_BLOCK', '48'))
    _PS_RETUNE_EVERY = int(os.environ.get('AMS_PS_RETUNE_EVERY', '50000'))       # replays between two measurements (0 = decide once)

    def _ps_finish_tuning(self, st):
        """Median step time (replay + optimizer, device events) of the two captured forms over the counted tuning steps; the faster
        form stays, the other graph is dropped.  The decision is kept on the model (a re-capture -- an audit, a restore -- reuses it)
        and published in K.PS_TUNED for reports."""
        tune = st['tune']
        torch.cuda.synchronize()
        med = []
        for v in (0, 1):
            t = sorted(a.elapsed_time(b) for i, a, b in tune['ev'][v] if i >= 2 * self._PS_TUNE_BLOCK // 3)
            med.append(t[len(t) // 2])
        keep = 0 if med[0] <= med[1] else 1
        st['graph'], st['cost'], st['run'] = tune['variants'][keep]
        st['tune'] = None
        self._ps_choice = (keep == 0)
        K.PS_TUNED.update(presplit=self._ps_choice, ms_presplit=round(med[0], 4), ms_in_product=round(med[1], 4), decisions=K.PS_TUNED.get('decisions', 0) + 1,
                          steps_counted=len([1 for i, a, b in tune['ev'][0] if i >= 2 * self._PS_TUNE_BLOCK // 3]))

    def _backward(self, cost):
        """d cost[0]: a 1-element cost is seeded with a cached ones tensor (no select / fill launches on the way back)."""
        K.flush_deferred_zero()          # zero_grad(defer=True): zeroed by pass_begin() on the side stream, or here if no pass began
        if cost.is_cuda:
            K.await_pass_side()          # gradients written on this stream come after that memset
        c = cost.reshape(-1)
        if c.numel() != 1:
            c[0].backward()
            return
        seed = self.__dict__.get('_seed')
        if seed is None or seed.device != c.device:
            seed = self.__dict__['_seed'] = torch.ones(1, dtype=c.dtype, device=c.device)
        c.backward(seed)

    def train(self, feed_dict, step):
        if self.args.get('hip_graph'):
            c = self._train_graphed(feed_dict, step)
            if c is not None:
                return c
        run = self._feeds(feed_dict, True)
        opt = self.optimize
        opt.zero_grad(defer=True)
        cost = self.cost_model.value(run)
        self._backward(cost)
        F.OVERLAP.join()
        opt.step()
        if self.summaries_enabled and getattr(self, 'merged_train', None):
            with torch.no_grad():
                self.train_writer.add(step, self._summaries(run, self.merged_train))
        self.last_run = run
        return cost.detach().reshape(-1)[0]

    def train_audited(self, feed_dict, step):
        """One training step, EAGER, with the fp16x3 range audit on (K.F16_AUDIT): every product launched with operand bounds also
        measures how much of each operand lies below bound * 2^-17.  A product class whose lost bits exceed the f32 level is sent back
        to bf16x6 from then on; a captured step is dropped so that the next call re-captures without it.  Returns (cost, newly denied)."""
        K.F16_AUDIT.begin()
        hg, self.args['hip_graph'] = self.args.get('hip_graph'), False
        try:
            c = self.train(feed_dict, step)
        finally:
            self.args['hip_graph'] = hg
            new = K.F16_AUDIT.finish()
        if new:
            self.__dict__.pop('_cg_state', None)
        return c, new

    # ---- a recurrence ring that could not get all its workgroups resident gives up a bounded wait and flags it in the device's
    # sticky error word (csrc/lstm_ring.hip, K.ring_error_word): the batch is then REPEATED on the per-step recurrence kernels,
    # which need no co-residency -- safe rather than loud.  `ring_fallbacks` counts how often that happened.
    ring_fallbacks = 0

    def _inputs_of(self, run):
        return [(n, n.value(run)) for n in (self.x_mix, self.x_non_mix, self.I)]

    def _eval_guarded(self, feed_dict, fn, training=False, inputs=None):
        """fn(run) without gradients; the same batch again on the per-step kernels when a ring launch gave up (one host sync: every
        caller reads its results on the host anyway).  inputs: (node, tensor) pairs that stand in for what the input pipeline would
        deliver (infer_chunks); a repeated batch sees the same tensors."""
        # a word that is ALREADY set belongs to an earlier (training) launch whose owner has yet to handle it (Trainer.train checks
        # right after the step): it is not this evaluation's to clear -- the batch is evaluated on the per-step kernels and the word
        # stays up
        pre = K.LSTM_RING != '0' and self._ring_error_any()
        run = self._feeds(feed_dict, training)
        for n, t in inputs or ():
            run.cache[id(n)] = t
        if not pre:
            with torch.no_grad():
                out = fn(run)
        # (pre: the word is up already -- a ring evaluation would be run, thrown away and leave nothing new to learn: straight to the
        # per-step kernels, one collective per batch instead of two)
        if K.LSTM_RING != '0' and (pre or self._ring_error_any()):
            # (every fed node is fed again: infer_chunks_masked also feeds the separator's masks)
            ins = self._inputs_of(run) + [(n, t) for n, t in inputs or () if all(n is not m for m in (self.x_mix, self.x_non_mix, self.I))]
            if not pre:
                K.ring_errors_clear()
            old, K.LSTM_RING = K.LSTM_RING, '0'
            try:
                run = self._feeds(feed_dict, training)
                for n, t in ins:
                    run.cache[id(n)] = t
                with torch.no_grad():
                    out = fn(run)
            finally:
                K.LSTM_RING = old
            Network.ring_fallbacks += 1
        return out

    def _ring_error_any(self):
        """Did a ring launch of the evaluation just run give up -- on ANY rank?  The decision to repeat a batch must be the same on
        every rank: the repeat may issue collectives (SparseKL all-reduces p_hat) its peers would otherwise not match."""
        d = self.dist
        if d is not None and getattr(d, 'enabled', False) and torch.cuda.is_available():
            d.all_reduce_max(K.ring_error_word())
        return K.ring_error_pending()

    def retrain_last(self, step):
        """Repeat the LAST training step on the per-step recurrence kernels.  Call when K.ring_error_pending() after train():
        the fused optimizer has skipped that step's update (the error word is its guard), so weights and slots are those of before
        the step; this runs the same batch eagerly with the ring off and applies the update.  Returns the cost."""
        run0 = self.last_run
        ins = self._inputs_of(run0)
        opt = self.optimize
        K.ring_errors_clear()
        opt.undo_counters()
        old, K.LSTM_RING = K.LSTM_RING, '0'
        try:
            run = Run(dict(run0.feeds), True)
            for n, t in ins:
                run.cache[id(n)] = t
            opt.zero_grad()
            cost = self.cost_model.value(run)
            self._backward(cost)
            F.OVERLAP.join()
            opt.step()
        finally:
            K.LSTM_RING = old
        Network.ring_fallbacks += 1
        self.last_run = run
        return cost.detach().reshape(-1)[0]

    def infer(self, feed_dict, step):
        return self._eval_guarded(feed_dict, lambda run: [self.x_mix.value(run), self.x_non_mix.value(run), self.output.value(run)])

    # ---- whole recordings: chunk, separate every chunk, track the outputs across the chunk borders, cross-fade
    def _refuse_unless_separating(self):
        if getattr(self, 'output', None) is None:
            raise ValueError('this model has no `output`: build it with an inference recipe (utils/trainer.py)')
        if getattr(self, 'pretraining', False):
            raise ValueError('a pretraining model separates with masks made from the clean sources (Adapt.separator): it cannot '
                             'separate a recording that comes without them')

    def infer_chunks(self, mix, batch_size=None):
        """mix [C, L] -> est [C, S, L]: `output` for every chunk, batch_size chunks per pass (default: the model's batch size).  The clean
        sources and the speaker indices a training pass would read are fed as zeros.  A short last batch is filled up with copies of
        its last chunk, which are dropped again: every pass has the same shape and the same k-means seed-draw pattern."""
        self._refuse_unless_separating()
        B = int(batch_size or self.args['batch_size'])
        if mix.dim() != 2 or mix.shape[1] != self.args['chunk_size']:
            raise ValueError('infer_chunks: chunks of %s samples for a model built with chunk_size %d'
                             % (tuple(mix.shape)[1:], self.args['chunk_size']))
        if B < 1 or mix.shape[0] < 1:
            raise ValueError('infer_chunks: needs at least one chunk and a batch size of at least 1')
        C, L = mix.shape
        xn = torch.zeros((B, self.S, L), dtype=mix.dtype, device=mix.device)
        ind = torch.zeros((B, self.S), dtype=torch.int32, device=mix.device)
        est = None
        for b0 in range(0, C, B):
            xm = mix[b0:b0 + B]
            n = xm.shape[0]
            if n < B:
                xm = torch.cat([xm, xm[-1:].expand(B - n, L)], dim=0)
            ins = [(self.x_mix, xm.contiguous()), (self.x_non_mix, xn), (self.I, ind)]
            out = self._eval_guarded({}, lambda run: self.output.value(run), inputs=ins)
            if est is None:
                if tuple(out.shape) != (B, self.S, L):
                    # (an STFT recipe returns the samples its frames cover: chunk_size must be window_size + k * hop_size)
                    raise ValueError('infer_chunks: `output` is %s, expected [%d, %d, %d]: the model must return every sample of a '
                                     'chunk' % (tuple(out.shape), B, self.S, L))
                est = torch.empty((C, self.S, L), dtype=out.dtype, device=out.device)
            est[b0:b0 + n] = out[:n]
        return est

    # ---- live streams: the same chunks, borders and cross-fade, one chunk behind samples that arrive block by block
    def open_streams(self, n, hop=None, batch_size=None):
        """-> ams_hip.stream.StreamSeparator for n parallel streams of mono float32 samples at config.fs: push(blocks) takes a block of any
        size per stream and returns what has become final, one chunk (chunk_size samples) behind; close(s) returns the rest.  The ready
        chunks of ALL streams of a push go through infer_chunks together, in passes of batch_size rows (default: the model's batch size),
        and are tracked and cross-faded by kernels whose launch count does not depend on n (include/ams_stream.h).  Only the default
        clustering='chunk' of separate_recording can run this way: it is causal in chunk order.

        A chunk's k-means seeds depend on the pass and the row of the batch it lands in (as in separate_recordings), and
        here that is decided by how the blocks arrive: a stream's output is DEFINED as ams_hip.stitch.stitch of the estimates its chunks
        got, bit for bit.  It equals separate_recording of the same samples only where those estimates are equal."""
        from ams_hip import stitch as St
        from ams_hip import stream as Sm
        self._refuse_unless_separating()
        L = int(self.args['chunk_size'])
        H = St.default_hop(L) if hop is None else int(hop)
        St.check_geometry(L, H)
        if int(n) < 1:
            raise ValueError('open_streams: at least one stream, got %d' % n)
        if batch_size is not None and int(batch_size) < 1:
            raise ValueError('open_streams: a batch size of at least 1, got %d' % batch_size)
        return Sm.StreamSeparator(lambda mix: self.infer_chunks(mix, batch_size), int(n), self.S, L, H, device=get_default_graph().device)

    # ---- recording-level clustering: the embeddings of ALL chunks of a recording are one point set for one k-means,
    # so every chunk shares its centroids and the labels mean the same speaker everywhere: no border permutation is left to decide
    CLUSTER_CAP_BYTES = 8 << 30                # packed points (Ctot TF E 4 bytes) clustered at a time, unless the caller says otherwise

    def _clustering_separator(self):
        """(separator, its KMeans) of a model that separates by k-means on embeddings; ValueError otherwise."""
        sep = getattr(self, 'sepNet', None) or self
        km = getattr(sep, 'kmeans', None)
        if km is None or getattr(sep, 'embeddings', None) is None or getattr(sep, 'masks', None) is None:
            raise ValueError("clustering='recording' needs a model with a k-means separator (`separate` on embeddings); this one has none")
        return sep, km

    def _check_speakers(self, clustering, speakers, min_score):
        """The refusals of `speakers`, all before anything is uploaded.  Returns None (the model's fixed S) or
        (lo, hi, min_score)."""
        if speakers is None:
            if min_score is not None:
                raise ValueError("min_score belongs to speakers='auto' or (lo, hi); without `speakers` every recording has the model's %d"
                                 % self.S)
            return None
        from ams_hip import spk_count as Sc
        lo, hi = Sc.parse_speakers(speakers, self.S)
        if clustering != 'recording':
            raise ValueError("speakers=%r needs clustering='recording': the count is chosen on the embeddings of a whole recording"
                             % (speakers,))
        sep, km = self._clustering_separator()
        if km.beta is not None:
            raise ValueError("speakers=%r is hard assignment only: this model runs a soft k-means (beta_kmeans = %r)" % (speakers, km.beta))
        if hasattr(sep, '_cache_enhance'):
            raise ValueError("speakers=%r with an enhance layer is not built: its softmax over the %d tracks would put energy into the "
                             "tracks a recording of fewer speakers leaves empty" % (speakers, self.S))
        Sc.check_range(lo, hi, self.S, min_score, getattr(sep, 'embedding_size', None))
        return lo, hi, None if min_score is None else float(min_score)

    def _check_clustering(self, clustering, kmeans_init_indices, R):
        """The refusals of the clustering arguments, all before anything is uploaded.  Returns the seeds as a list of R int32 [tries, C]
        host arrays (None: to be drawn)."""
        if clustering not in ('chunk', 'recording', 'recording_soft'):
            raise ValueError("clustering must be 'chunk' or 'recording' (or 'recording_soft' on a soft k-means model), got %r" % (clustering,))
        if clustering == 'chunk':
            if kmeans_init_indices is not None:
                raise ValueError("kmeans_init_indices are the per-recording seeds of clustering='recording'; the per-chunk seeds of "
                                 "clustering='chunk' belong to the model (--kmeans_init_indices)")
            return None
        sep, km = self._clustering_separator()
        if clustering == 'recording' and km.beta is not None:
            raise ValueError("clustering='recording' is hard assignment only: this model runs a soft k-means (beta_kmeans = %r); its "
                             "recording-level mode is clustering='recording_soft'" % (km.beta,))
        if clustering == 'recording_soft' and km.beta is None:
            raise ValueError("clustering='recording_soft' needs a model with a soft k-means (beta_kmeans set): this one assigns hard "
                             "(beta_kmeans = None) and takes clustering='recording'")
        if kmeans_init_indices is None:
            return None
        seeds = list(kmeans_init_indices) if hasattr(kmeans_init_indices, '__len__') and not torch.is_tensor(kmeans_init_indices) else None
        if seeds is None or len(seeds) != R:
            raise ValueError('kmeans_init_indices: a list of one [tries, clusters] array per recording (%d), got %s'
                             % (R, type(kmeans_init_indices).__name__ if seeds is None else 'a list of %d' % len(seeds)))
        out = []
        for r, v in enumerate(seeds):
            v = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
            if v.dtype.kind not in 'iu' or v.shape != (km.nb_tries, km.nb_clusters):
                raise ValueError('kmeans_init_indices[%d]: integers of shape [tries, clusters] = [%d, %d], got %s %s'
                                 % (r, km.nb_tries, km.nb_clusters, v.dtype, v.shape))
            out.append(v.astype(np.int32))
        return out

    def _check_seeding(self, clustering, recording_seeding, kmeans_seed_draws, kmeans_init_indices, R):
        """The refusals of the seeding arguments, all before anything is uploaded.  Returns None ('model': the seeds
        are the caller's or the model's own draw) or, for 'plusplus', a list of R entries: the caller's uint64 [tries, clusters] draws of
        every recording, or None each where the model's KMeans is to draw them."""
        if recording_seeding not in ('model', 'plusplus'):
            raise ValueError("recording_seeding must be 'model' or 'plusplus', got %r" % (recording_seeding,))
        if recording_seeding == 'model':
            if kmeans_seed_draws is not None:
                raise ValueError("kmeans_seed_draws are the random numbers of recording_seeding='plusplus'; the seeds of "
                                 "recording_seeding='model' are kmeans_init_indices")
            return None
        if clustering == 'chunk':
            raise ValueError("recording_seeding='plusplus' seeds the k-means of a whole recording: it needs clustering='recording' or "
                             "'recording_soft' (the per-chunk seeds of clustering='chunk' belong to the model)")
        if kmeans_init_indices is not None:
            raise ValueError("recording_seeding='plusplus' chooses the seeds itself: kmeans_init_indices cannot be given with it")
        sep, km = self._clustering_separator()
        if kmeans_seed_draws is None:
            return [None] * R
        draws = list(kmeans_seed_draws) if hasattr(kmeans_seed_draws, '__len__') and not torch.is_tensor(kmeans_seed_draws) else None
        if draws is None or len(draws) != R:
            raise ValueError('kmeans_seed_draws: a list of one uint64 [tries, clusters] array per recording (%d), got %s'
                             % (R, type(kmeans_seed_draws).__name__ if draws is None else 'a list of %d' % len(draws)))
        out = []
        for r, v in enumerate(draws):
            v = np.asarray(v) if not torch.is_tensor(v) else None
            if v is None or v.dtype != np.uint64 or v.shape != (km.nb_tries, km.nb_clusters):
                raise ValueError('kmeans_seed_draws[%d] (recording %d): a host uint64 array of shape [tries, clusters] = [%d, %d], got %s'
                                 % (r, r, km.nb_tries, km.nb_clusters, 'a tensor' if v is None else '%s %s' % (v.dtype, v.shape)))
            out.append(np.ascontiguousarray(v))
        return out

    def _chunk_batches(self, mix, batch_size, what):
        """The batches infer_chunks makes of mix [C, L]: (first chunk, chunks that count, the fed inputs) per model pass."""
        self._refuse_unless_separating()
        B = int(batch_size or self.args['batch_size'])
        if mix.dim() != 2 or mix.shape[1] != self.args['chunk_size']:
            raise ValueError('%s: chunks of %s samples for a model built with chunk_size %d'
                             % (what, tuple(mix.shape)[1:], self.args['chunk_size']))
        if B < 1 or mix.shape[0] < 1:
            raise ValueError('%s: needs at least one chunk and a batch size of at least 1' % what)
        C, L = mix.shape
        xn = torch.zeros((B, self.S, L), dtype=mix.dtype, device=mix.device)
        ind = torch.zeros((B, self.S), dtype=torch.int32, device=mix.device)
        for b0 in range(0, C, B):
            xm = mix[b0:b0 + B]
            n = xm.shape[0]
            if n < B:
                xm = torch.cat([xm, xm[-1:].expand(B - n, L)], dim=0)
            yield b0, n, [(self.x_mix, xm.contiguous()), (self.x_non_mix, xn), (self.I, ind)]

    def _embed_batches(self, mix, batch_size):
        """Pass 1, one model pass per batch: (first chunk, chunks that count, points [B, TF, E], weights [B, TF] or None).  The points
        are normalised exactly as the model's KMeans normalises them (ams_hip/kmeans_host.py: _run), the one-pass form of the Normalize
        layer and the k-means' own normalisation where it applies; the silence weights are per chunk, as there."""
        sep, km = self._clustering_separator()

        def points(run):
            if km.pre_norm is not None and km.normalize_input:
                node, E = km.pre_norm
                u = node.value(run)
                xn = K.l2norm_kmeans_normalize(F._c(u.reshape(u.shape[0], -1, E)), E)
            else:
                X = F._c(sep.embeddings.value(run))
                xn = K.kmeans_normalize(X) if km.normalize_input else X
            w = None
            if km.latent_space_tensor is not None:
                w = K.silence_weights(km.latent_space_tensor.value(run).reshape(xn.shape[0], xn.shape[1]).contiguous(), km.threshold)
            return xn, w
        for b0, n, ins in self._chunk_batches(mix, batch_size, 'embed_chunks'):
            xn, w = self._eval_guarded({}, points, inputs=ins)
            yield b0, n, xn, w

    def embed_chunks(self, mix, batch_size=None):
        """mix [C, L] -> (points [C, TF, E], weights [C, TF] or None): the separator's embeddings of every chunk as its k-means would
        see them (normalised; the silence weights where the model was built --with_silence), in the batches of infer_chunks."""
        pts = wts = None
        for b0, n, xn, w in self._embed_batches(mix, batch_size):
            if pts is None:
                pts = torch.empty((mix.shape[0],) + tuple(xn.shape[1:]), dtype=xn.dtype, device=xn.device)
                wts = None if w is None else torch.empty((mix.shape[0], xn.shape[1]), dtype=w.dtype, device=w.device)
            pts[b0:b0 + n] = xn[:n]
            if w is not None:
                wts[b0:b0 + n] = w[:n]
        return pts, wts

    def infer_chunks_masked(self, mix, masks, batch_size=None):
        """mix [C, L], masks [C, TF, S] -> est [C, S, L]: `output` for every chunk with the separator's `masks` node FED, in the batches of
        infer_chunks.  Neither the embedding network nor the k-means runs; the enhance layer and the back end follow the masks."""
        sep, _ = self._clustering_separator()
        if not torch.is_tensor(masks) or masks.dim() != 3 or masks.shape[0] != mix.shape[0] or masks.shape[2] != self.S:
            raise ValueError('infer_chunks_masked: masks [%d, TF, %d] for these chunks, got %s'
                             % (mix.shape[0], self.S, tuple(masks.shape) if torch.is_tensor(masks) else type(masks).__name__))
        est = None
        for b0, n, ins in self._chunk_batches(mix, batch_size, 'infer_chunks_masked'):
            mk = masks[b0:b0 + n]
            B = ins[0][1].shape[0]
            if n < B:
                mk = torch.cat([mk, mk[-1:].expand(B - n, mk.shape[1], mk.shape[2])], dim=0)
            out = self._eval_guarded({}, lambda run: self.output.value(run), inputs=ins + [(sep.masks, mk.contiguous())])
            if est is None:
                if tuple(out.shape) != (B, self.S, mix.shape[1]):
                    raise ValueError('infer_chunks_masked: `output` is %s, expected [%d, %d, %d]: the model must return every sample of '
                                     'a chunk' % (tuple(out.shape), B, self.S, mix.shape[1]))
                est = torch.empty((mix.shape[0], self.S, mix.shape[1]), dtype=out.dtype, device=out.device)
            est[b0:b0 + n] = out[:n]
        return est

    def _infer_chunks_clustered(self, mix, counts, seeds, batch_size, cap_bytes, speakers=None, soft=False, plusplus=None):
        """mix [Ctot, L]: the chunks of R recordings, counts[r] each, one after the other -> est [Ctot, S, L] with ONE k-means per
        recording over the embeddings of all its chunks.  2 ceil(Ctot / B) model passes whatever R is.  The points are held for a group
        of consecutive recordings at a time (at most cap_bytes of them); the model passes run over the WHOLE stream in the same
        batches whatever the groups are, and a recording is clustered on its own, so no result depends on the grouping.
        speakers = (lo, hi, min_score): every recording's number of clusters is chosen in lo .. hi (ams_hip/spk_count.py, DESIGN.md
        4.11); labels below the recording's count leave the other mask columns all-zero.
        soft (clustering='recording_soft'): the model's soft k-means (beta_kmeans) per recording
        (ams_hip/kmeans_ragged_soft.py); its soft labels are written straight into the [Ctot, TF, S] masks the second sweep is fed with,
        and last_clustering holds 'masks' instead of 'labels'.
        plusplus (recording_seeding='plusplus'): per recording the uint64 [tries, S] draws, or None where the model's KMeans
        draws them; the seeds of a group are chosen on the device from its points and the k-means' weights (ams_hip/kmeans_seed.py), copied
        to the host ONCE per group and handed to the same calls as the seeds of the other path; last_clustering holds them as 'seeds'."""
        from ams_hip import kmeans_ragged as Kr
        from ams_hip import kmeans_ragged_soft as Krs
        from ams_hip import kmeans_seed as Ks
        from ams_hip import spk_count as Sc
        sep, km = self._clustering_separator()
        cap = int(self.CLUSTER_CAP_BYTES if cap_bytes is None else cap_bytes)
        counts = [int(c) for c in counts]
        R, Ctot = len(counts), mix.shape[0]
        first = np.concatenate([[0], np.cumsum(counts)])
        labels = masks = cents = bests = None
        counted = {'counts': [], 'scores': [], 'tries': []}
        chosen = []                           # per group, the k-means++ seeds [recordings of the group, tries, S] on the device
        groups, g = None, 0                   # [(first recording, end recording)], the group being filled
        pts = wts = None

        def cluster(r0, r1):
            TF, E = pts.shape[1], pts.shape[2]
            seg = Kr.Segments([c * TF for c in counts[r0:r1]])
            # seeds per recording, in list order: the caller's, or the model's own draw (reference / fast / keyed) over the recording's points
            if plusplus is not None:
                # D^2 sampling on the device, once with the model's S clusters (a count below S takes the first columns); ONE copy of
                # R tries S int32 to the host per group, so that the calls below keep their host-side check of the seeds
                D = np.concatenate([plusplus[r] if plusplus[r] is not None else km.seed_draws(km.nb_tries, km.nb_clusters) for r in range(r0, r1)])
                sd = Ks.seed_plusplus(pts.view(-1, E), seg, km.nb_clusters, km.nb_tries, D, w=None if wts is None else wts.view(-1))
                chosen.append(sd.view(r1 - r0, km.nb_tries, km.nb_clusters))
                idx = sd.cpu().numpy()
            else:
                idx = np.concatenate([seeds[r] if seeds is not None else km._draw(km.nb_tries, counts[r] * TF).numpy() for r in range(r0, r1)])
            if speakers is not None:
                lo, hi, min_score = speakers
                res = Sc.count_clusters(pts.view(-1, E), seg, idx, lo, hi, km.nb_tries, km.nb_iterations,
                                        w=None if wts is None else wts.view(-1), assign_at_end=km.assign_at_end, normalize_input=False,
                                        min_score=min_score)
                labels[first[r0]:first[r1]] = res['labels'].view(-1, TF)
                cents.append(res['centroids'])
                # the chosen try of the chosen candidate (-1 for a recording of one speaker)
                cd = res['cand'].long()
                bests.append(torch.where(cd >= 0, res['tries'].gather(1, cd.clamp(min=0)[:, None])[:, 0], cd.to(torch.int32)))
                for key, name in (('counts', 'count'), ('scores', 'scores'), ('tries', 'tries')):
                    counted[key].append(res[name])
                return
            if soft:
                # the soft labels of the group's recordings go straight into their rows of the masks buffer
                c, _, b = Krs.kmeans_ragged_soft(pts.view(-1, E), seg, idx, km.nb_clusters, km.nb_tries, km.nb_iterations, km.beta,
                                                 w=None if wts is None else wts.view(-1), assign_at_end=km.assign_at_end,
                                                 normalize_input=False, out=masks[first[r0]:first[r1]])
                cents.append(c)
                bests.append(b)
                return
            c, lab, b = Kr.kmeans_ragged(pts.view(-1, E), seg, idx, km.nb_clusters, km.nb_tries, km.nb_iterations,
                                         w=None if wts is None else wts.view(-1), assign_at_end=km.assign_at_end, normalize_input=False)
            labels[first[r0]:first[r1]] = lab.view(-1, TF)
            cents.append(c)
            bests.append(b)

        for b0, n, xn, w in self._embed_batches(mix, batch_size):
            if groups is None:
                TF, E = xn.shape[1], xn.shape[2]
                if soft:
                    Krs.check_domain(E, km.nb_clusters, km.beta)
                    if km.nb_clusters != self.S:
                        raise ValueError("clustering='recording_soft': the k-means has %d clusters for %d sources" % (km.nb_clusters, self.S))
                elif speakers is None:
                    Kr.check_domain(E, km.nb_clusters)
                else:
                    Sc.check_range(speakers[0], speakers[1], self.S, speakers[2], E)
                if plusplus is not None:
                    Ks.check_domain(E, km.nb_clusters)
                    if speakers is not None and km.nb_clusters < speakers[1]:
                        raise ValueError("recording_seeding='plusplus': the k-means has %d clusters, fewer than the %d of speakers"
                                         % (km.nb_clusters, speakers[1]))
                per_chunk = TF * E * 4
                groups, r0, acc = [], 0, 0
                for r, c in enumerate(counts):
                    if c * per_chunk > cap:
                        raise ValueError('recording %d: %d chunks of %d points x %d floats are %d bytes of embeddings, above the cap of %d '
                                         'bytes (cluster_cap_bytes)' % (r, c, TF, E, c * per_chunk, cap))
                    if acc + c * per_chunk > cap:
                        groups.append((r0, r))
                        r0, acc = r, 0
                    acc += c * per_chunk
                groups.append((r0, R))
                if soft:
                    masks = torch.empty((Ctot, TF, self.S), dtype=torch.float32, device=xn.device)
                else:
                    labels = torch.empty((Ctot, TF), dtype=torch.int32, device=xn.device)
                cents, bests = [], []
            at = 0                           # rows of this batch handed out so far
            while at < n:
                r0, r1 = groups[g]
                c0, c1 = int(first[r0]), int(first[r1])
                if pts is None:
                    pts = torch.empty((c1 - c0,) + tuple(xn.shape[1:]), dtype=xn.dtype, device=xn.device)
                    wts = None if w is None else torch.empty((c1 - c0, xn.shape[1]), dtype=w.dtype, device=w.device)
                k = min(n - at, c1 - (b0 + at))
                pts[b0 + at - c0:b0 + at - c0 + k] = xn[at:at + k]
                if w is not None:
                    wts[b0 + at - c0:b0 + at - c0 + k] = w[at:at + k]
                at += k
                if b0 + at == c1:
                    cluster(r0, r1)
                    pts = wts = None
                    g += 1
        self.last_clustering = {'centroids': torch.cat(cents), 'best': torch.cat(bests), 'first_chunk': first, 'groups': groups}
        self.last_clustering['masks' if soft else 'labels'] = masks if soft else labels
        if speakers is not None:
            self.last_clustering.update({k: torch.cat(v) for k, v in counted.items()})
        if plusplus is not None:
            self.last_clustering['seeds'] = torch.cat(chosen)
        return self.infer_chunks_masked(mix, masks if soft else F.one_hot_masks(labels, self.S), batch_size)

    def separate_recording(self, x, hop=None, batch_size=None, fs=None, output_fs=None, clustering='chunk', kmeans_init_indices=None,
                           cluster_cap_bytes=None, speakers=None, min_score=None, recording_seeding='model', kmeans_seed_draws=None):
        """x [N] (a tensor or anything numpy takes) -> out [S, N] on the device: chunks of the model's chunk_size, `hop` apart (default
        half a chunk), separated by infer_chunks and put together by ams_hip.stitch (include/ams_stitch.h).

        clustering='recording' (DESIGN.md 4.10): ONE hard k-means over the embeddings of all chunks of the recording (TF points per chunk;
        a frame in the overlap of two chunks is two points) instead of one per chunk, then the cross-fade with the identity track table:
        no border statistics, no tracker.  kmeans_init_indices: [seeds [tries, clusters]] over the recording's C TF points (default: the
        model's own draw); cluster_cap_bytes: see separate_recordings.  The default 'chunk' is the path described above, unchanged.

        clustering='recording_soft' (DESIGN.md 4.13): the same for a model with a SOFT k-means (beta_kmeans set; 'recording' refuses it,
        and this mode refuses a hard model): one soft k-means over the recording's points (ams_hip.kmeans_ragged_soft), whose soft
        labels are the masks of every chunk.  kmeans_init_indices and cluster_cap_bytes as for 'recording'; `speakers` is not built for
        it.  last_clustering then holds 'masks' [C, TF, S] instead of 'labels'.

        speakers='auto' (= (2, S)) or (lo, hi), with clustering='recording' (DESIGN.md 4.11): the number of speakers S_r of the recording
        is chosen in lo .. hi by the simplified silhouette of the k-means of every candidate count, and out is [S_r, N], the first S_r
        tracks.  lo == 1 needs min_score: the score below which the recording counts as one speaker.  last_clustering then also
        holds 'counts', 'scores' and 'tries'.  How well the criterion counts speakers on a trained model has not been measured.

        recording_seeding='plusplus' (DESIGN.md 4.14), with 'recording' or 'recording_soft': the seeds of every try are chosen on the device
        by k-means++ (D^2 sampling with integer weights, ams_hip.kmeans_seed) from the recording's points and the k-means' weights instead of
        uniformly, copied to the host once and handed to the same k-means; with `speakers` the seeding is made once for the model's S
        clusters and every candidate count takes its first columns.  kmeans_seed_draws: [uint64 [tries, clusters]], the random numbers
        (default: the stream of the model's KMeans, seed_draws); not together with kmeans_init_indices.  last_clustering then also holds
        'seeds' [1, tries, S].  The default 'model' is the path described above, every bit unchanged.

        fs: the sample rate of x (default config.fs, the rate the models work at).  At another rate -- or for int16 frames [N, CH], which
        are decoded and mixed down -- x is brought to config.fs on the device (ams_hip.resample, include/ams_resample.h), separated as
        above, and the [S, M] result is resampled to output_fs (default fs) and cut to ceil(N output_fs / fs) samples: N at the rate of
        the input.  Nothing goes through the host between the upload and the result."""
        from ams_hip import stitch as St
        self._refuse_unless_separating()
        L = int(self.args['chunk_size'])
        H = St.default_hop(L) if hop is None else int(hop)
        St.check_geometry(L, H)
        fs_in = config.fs if fs is None else int(fs)
        fs_out = fs_in if output_fs is None else int(output_fs)
        pcm = (x.dtype == torch.int16) if torch.is_tensor(x) else (getattr(x, 'dtype', None) == np.int16)
        seeds = self._check_clustering(clustering, kmeans_init_indices, 1)
        spk = self._check_speakers(clustering, speakers, min_score)
        pp = self._check_seeding(clustering, recording_seeding, kmeans_seed_draws, kmeans_init_indices, 1)
        if pcm or fs_in != config.fs or fs_out != config.fs:
            return self._separate_resampled(x, pcm, H, batch_size, fs_in, fs_out, clustering, kmeans_init_indices, cluster_cap_bytes,
                                            speakers, min_score, recording_seeding, kmeans_seed_draws)
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        x = x.to(device=get_default_graph().device, dtype=torch.float32).contiguous()
        if x.dim() != 1 or x.shape[0] < 1:
            raise ValueError('separate_recording: one channel of at least one sample, got %s' % (tuple(x.shape),))
        if clustering != 'chunk':
            mix = St.chunks(x, L, H)
            est = self._infer_chunks_clustered(mix, [mix.shape[0]], seeds, batch_size, cluster_cap_bytes, spk, soft=clustering == 'recording_soft',
                                               plusplus=pp)
            trk = torch.arange(self.S, dtype=torch.int32, device=est.device).repeat(mix.shape[0], 1)       # the identity: nothing to track
            out = St.overlap_add(est, trk, x.shape[0], H)
            return out if spk is None else out[:int(self.last_clustering['counts'][0])]
        est = self.infer_chunks(St.chunks(x, L, H), batch_size)
        return St.stitch(est, x.shape[0], H)[0]

    def _separate_resampled(self, x, pcm, H, batch_size, fs_in, fs_out, clustering='chunk', kmeans_init_indices=None, cluster_cap_bytes=None,
                            speakers=None, min_score=None, recording_seeding='model', kmeans_seed_draws=None):
        from ams_hip import resample as Rs
        Rs.ratio(fs_in, config.fs)                                 # a ValueError before anything is uploaded
        Rs.ratio(config.fs, fs_out)
        if not torch.is_tensor(x):
            x = torch.from_numpy(np.array(x, dtype=np.int16 if pcm else np.float32))      # (a copy: frames read from a file are read-only)
        x = x.to(device=get_default_graph().device, dtype=torch.int16 if pcm else torch.float32).contiguous()
        if pcm and x.dim() == 1:
            x = x.reshape(-1, 1)
        if x.dim() != (2 if pcm else 1) or x.shape[0] < 1:
            raise ValueError('separate_recording: float32 [N] or int16 frames [N, CH] of at least one sample, got %s %s'
                             % (x.dtype, tuple(x.shape)))
        N = x.shape[0]
        x = Rs.from_pcm16(x, fs_in, config.fs) if pcm else Rs.resample(x, fs_in, config.fs)
        out = self.separate_recording(x, hop=H, batch_size=batch_size, clustering=clustering, kmeans_init_indices=kmeans_init_indices,
                                      cluster_cap_bytes=cluster_cap_bytes, speakers=speakers, min_score=min_score,
                                      recording_seeding=recording_seeding, kmeans_seed_draws=kmeans_seed_draws)
        if fs_out == config.fs:
            return out
        out = Rs.resample(out, config.fs, fs_out)
        n_out = -((-N * fs_out) // fs_in)                          # <= out.shape[1]: the way back yields ceil(M fs_out / config.fs)
        return out[:, :n_out].contiguous() if n_out < out.shape[1] else out

    def separate_recordings(self, xs, hop=None, batch_size=None, fs=None, output_fs=None, clustering='chunk', kmeans_init_indices=None,
                            cluster_cap_bytes=None, speakers=None, min_score=None, recording_seeding='model', kmeans_seed_draws=None):
        """xs: a list of recordings, float32 [N_r] each (tensors or anything numpy takes) -> a list of [S, N_r] device tensors.  The chunks
        of ALL recordings go through infer_chunks as one stream -- ceil(Ctot / batch_size) model passes instead of one or more per
        recording -- and are cut, tracked and cross-faded by kernels whose launch count does not depend on len(xs)
        (ams_hip.stitch_batch, include/ams_stitch_batch.h).  The results are views of one packed buffer.

        A chunk's k-means seeds depend on the row of the batch it sits in (kmeans_init_indices has a row per batch row and try), and here
        a chunk's row is its place in the stream: separate_recordings(xs)[r] is DEFINED as the stitch of the batched inference.  It is not
        bit-equal to separate_recording(xs[r]) -- except for a single recording, where the rows coincide.

        fs / output_fs as in separate_recording, for float32 [N_r] or int16 frames [N_r, CH_r] (all of one dtype; CH_r may differ).  fs is
        one rate for all recordings or a sequence of len(xs) rates; output_fs is None (every recording comes back at its own fs), one rate,
        or a sequence of len(xs) rates.  All recordings are decoded, mixed down and brought to config.fs in ONE launch, written straight
        into the packed buffer the chunks are cut from, and go back to their output rates, cut to ceil(N_r output_fs_r / fs_r) samples,
        in ONE launch (ams_hip.resample_ragged, include/ams_resample_ragged.h): recordings of different rates share one
        chunk stream.  Every recording's conversion is bit-equal to separate_recording's (ams_hip.resample) on it alone; the results are
        views of one buffer.  A rate the resampler refuses is a ValueError that names the recording (with a sequence) before any upload.

        clustering='recording' (DESIGN.md 4.10): one hard k-means per recording over the embeddings of all its chunks -- all recordings in
        ONE ragged call (ams_hip.kmeans_ragged) between two sweeps of the chunk stream, 2 ceil(Ctot / batch_size) model passes -- and the
        cross-fade with the identity track table.  kmeans_init_indices: one [tries, clusters] array per recording, over its C_r TF points
        (default: the model's own draw, per recording in list order).  cluster_cap_bytes (default CLUSTER_CAP_BYTES = 8 GiB): the
        embeddings are held for a group of consecutive recordings of at most that many bytes at a time; a recording's result does not
        depend on the grouping; a single recording above the cap is refused.

        clustering='recording_soft' (DESIGN.md 4.13): the same for a model with a soft k-means (beta_kmeans set): all recordings in ONE
        ragged soft call per group (ams_hip.kmeans_ragged_soft), the soft labels written straight into the masks of the second sweep;
        every recording is bit-equal to separate_recording on it alone with the same seeds.  Not with `speakers`.

        speakers / min_score as in separate_recording: every recording gets its own number of speakers S_r, chosen for all recordings in
        one counted call whose launches do not depend on len(xs), and its result is [S_r, N_r].

        recording_seeding / kmeans_seed_draws as in separate_recording: one uint64 [tries, clusters] array per recording (default: drawn
        per recording in list order); the seeds of all recordings of a group are chosen in one call whose launches do not depend on
        len(xs), and one copy of R tries S int32 per group brings them to the host.  last_clustering['seeds'] is [R, tries, S]."""
        from ams_hip import stitch as St
        from ams_hip import stitch_batch as Sb
        self._refuse_unless_separating()
        if isinstance(xs, (torch.Tensor, np.ndarray)) or not hasattr(xs, '__len__'):
            raise ValueError('separate_recordings: a list of recordings, got %s (one recording: separate_recording)' % type(xs).__name__)
        xs = list(xs)
        if not xs:
            raise ValueError('separate_recordings: an empty list of recordings')
        seeds = self._check_clustering(clustering, kmeans_init_indices, len(xs))
        spk = self._check_speakers(clustering, speakers, min_score)
        pp = self._check_seeding(clustering, recording_seeding, kmeans_seed_draws, kmeans_init_indices, len(xs))
        L = int(self.args['chunk_size'])
        H = St.default_hop(L) if hop is None else int(hop)
        St.check_geometry(L, H)
        fs_in, fs_out = self._rates(fs, output_fs, len(xs))
        xs = [x if torch.is_tensor(x) else np.asarray(x) for x in xs]
        kinds = set(str(x.dtype).replace('torch.', '') for x in xs)
        if len(kinds) > 1:
            raise ValueError('separate_recordings: recordings of one dtype, got %s' % sorted(kinds))
        if kinds - {'int16', 'float32'}:
            raise ValueError('separate_recordings: float32 [N] or int16 frames [N, CH], got %s' % sorted(kinds))
        pcm = kinds == {'int16'}
        for x in xs:
            if x.ndim not in ((1, 2) if pcm else (1,)) or x.shape[0] < 1:
                raise ValueError('separate_recordings: float32 [N] or int16 frames [N, CH] of at least one sample, got %s %s'
                                 % (x.dtype, tuple(x.shape)))
        resampled = pcm or any(f != config.fs for f in fs_in + fs_out)
        if resampled:
            from ams_hip import resample as Rs
            from ams_hip import resample_ragged as Rr
            named = any(v is not None and not np.isscalar(v) for v in (fs, output_fs))
            for r in range(len(xs) if named else 1):               # a ValueError before anything is uploaded; a list names the recording
                try:
                    Rs.ratio(fs_in[r], config.fs)
                    Rs.ratio(config.fs, fs_out[r])
                except ValueError as e:
                    raise ValueError('recording %d: %s' % (r, e)) if named else e
            lengths = [x.shape[0] for x in xs]
        device = get_default_graph().device
        if resampled:
            # ONE launch for all recordings' decode, down-mix and rate conversion, straight into the packed buffer of the layout
            xp, lay = Rr.to_model_rate(xs, fs_in, L=L, H=H, S=self.S, device=device, fs_model=config.fs)
            mix = Sb.chunks_packed(xp, lay)
        elif all(torch.is_tensor(x) and x.is_cuda for x in xs):
            mix, lay = Sb.chunks_many([x.contiguous() for x in xs], L, H, self.S)
        else:
            # recordings on the host: packed there and uploaded once
            lay = Sb.layout([x.shape[0] for x in xs], L, H, self.S)
            host = np.zeros(lay.x_total, np.float32)
            for x, o, n in zip(xs, lay.x_off, lay.n):
                host[o:o + n] = x.detach().cpu().numpy() if torch.is_tensor(x) else x
            mix = Sb.chunks_packed(torch.from_numpy(host).to(device), lay)
        if clustering != 'chunk':
            est = self._infer_chunks_clustered(mix, lay.C.tolist(), seeds, batch_size, cluster_cap_bytes, spk, soft=clustering == 'recording_soft',
                                               plusplus=pp)
            trk = torch.arange(self.S, dtype=torch.int32, device=est.device).repeat(lay.Ctot, 1)          # the identity: nothing to track
            out = Sb.overlap_add_many(est, trk, lay)
            outs = [out[int(o):int(o) + self.S * int(n)].view(self.S, int(n)) for o, n in zip(lay.out_off, lay.n)]
            if spk is not None:
                outs = [o[:int(c)] for o, c in zip(outs, self.last_clustering['counts'].tolist())]       # the first S_r tracks
        else:
            out, res = Sb.stitch_many(self.infer_chunks(mix, batch_size), lay, packed=True)
            outs = [o for o, _, _ in res]
        if not resampled or all(f == config.fs for f in fs_out):
            return outs
        # ONE launch for all recordings' way back, cut to ceil(N output_fs / fs) samples: N at the rate of the input (the rule of
        # _separate_resampled; never more than the way back yields)
        keep = [min(-((-N * fo) // fi), Rs.out_len(int(n), *Rs.ratio(config.fs, fo))) for N, fi, fo, n in zip(lengths, fs_in, fs_out, lay.n)]
        return Rr.from_model_rate(out, lay, [o.shape[0] for o in outs], fs_out, keep, fs_model=config.fs)

    @staticmethod
    def _rates(fs, output_fs, R):
        """(fs_in [R], fs_out [R]) from the fs / output_fs of separate_recordings: None, one rate, or a sequence of R rates."""
        def many(v, name):
            if np.isscalar(v):
                v = [v] * R
            v = list(v)
            if len(v) != R:
                raise ValueError('separate_recordings: %s has %d rates for %d recordings' % (name, len(v), R))
            for f in v:
                if not isinstance(f, (int, float, np.integer, np.floating)) or isinstance(f, bool) or int(f) != f:
                    raise ValueError('separate_recordings: %s: a sample rate is an integer, got %r' % (name, f))
            return [int(f) for f in v]
        fs_in = [config.fs] * R if fs is None else many(fs, 'fs')
        return fs_in, (list(fs_in) if output_fs is None else many(output_fs, 'output_fs'))

    def improvement(self, feed_dict, step):
        return self._eval_guarded(feed_dict, lambda run: [self.x_mix.value(run), self.x_non_mix.value(run), self.sdr_imp.value(run)])

    def valid_batch(self, feed_dict, step):
        def fn(run):
            cost = self.cost_model.value(run)
            return run, float(cost.reshape(-1)[0].item())
        run, c = self._eval_guarded(feed_dict, fn)
        if getattr(self, 'merged_valid', None) and self.summaries_enabled:
            with torch.no_grad():
                self.valid_writer.add(step, self._summaries(run, self.merged_valid))
        return c

    def get_embeddings(self, feed_dict):
        return self._eval_guarded(feed_dict, lambda run: self.prediction.value(run))

    def test_batch(self, feed_dict):
        return self._eval_guarded(feed_dict, lambda run: float(self.cost_model.value(run).reshape(-1)[0].item()))

    def test(self, feed_dict):
        run = self._feeds(feed_dict, True)
        with torch.no_grad():
            return self.y.value(run)

    def add_valid_summary(self, val, step):
        self.valid_writer.add(step, {'Valid Cost': float(val)})

    def freeze_all_with(self, prefix):
        self.trainable_variables = [v for v in self.trainable_variables if prefix not in v.ams_name]

    def freeze_all_except(self, *prefix):
        to_train = []
        for var in self.trainable_variables:
            for p in prefix:
                if p in var.ams_name:
                    to_train.append(var)
                    break
        self.trainable_variables = to_train

    @classmethod
    def load(cls, path, modified_args):
        # Load parameters used for the desired model to load (network.py:291-306)
        params_path = os.path.join(path, 'params')
        with open(params_path) as f:
            args = json.load(f)
            keys_to_update = ['learning_rate', 'epochs', 'batch_size', 'chunk_size', 'nb_speakers',
                              'regularization', 'overlap_coef', 'loss', 'beta', 'model_folder', 'type', 'pretraining',
                              'with_silence', 'end_assign', 'beta_kmeans', 'nb_tries', 'nb_steps', 'threshold', 'optimizer',
                              'men', 'women', 'recurrent_dropout', 'recurrent_dropout_enhance',
                              # this build's own switches follow the CURRENT command line, not the loaded model's
                              'hip_graph', 'no_summaries', 'summaries', 'synthetic_batches', 'synthetic_pool', 'run_id',
                              'kmeans_seeding', 'f16_audit_every', 'dist']
            to_modify = {key: modified_args[key] for key in keys_to_update if key in modified_args.keys()}
            to_modify.update({key: val for key, val in modified_args.items() if key not in args.keys()})
        args.update(to_modify)
        print("LOADED = ", {k: v for k, v in args.items() if _jsonable(v)})
        return cls(**args)

    def finish_construction(self):
        self.trainable_variables = get_default_graph().global_variables()


def _jsonable(v):
    try:
        json.dumps(v)
        return True
    except (TypeError, ValueError):
        return False


from models.Kmeans_2 import KMeans  # noqa: E402  (reference import order, network.py:311)


class Separator(Network):

    def __init__(self, plugged=False, *args, **kwargs):
        super(Separator, self).__init__(plugged, *args, **kwargs)

        self.num_speakers = kwargs['tot_speakers']
        self.layer_size = kwargs['layer_size']
        self.embedding_size = kwargs['embedding_size']
        self.normalize = kwargs['no_normalize']
        self.nb_layers = kwargs['nb_layers']
        self.a = kwargs['mask_a']
        self.b = kwargs['mask_b']
        self.rdropout = kwargs['recurrent_dropout']

        # Preproc
        self.normalize_input = kwargs['normalize_separator']
        self.abs_input = kwargs['abs_input']
        self.pre_func = kwargs['pre_func']
        self.silent_threshold = kwargs['silence_mask_db']

        # Loss Parameters
        self.loss_with_silence = kwargs['silence_loss']
        self.threshold_silence_loss = kwargs['threshold_silence_loss']
        self.function_mask = kwargs['function_mask']

        # Kmeans Parameters
        self.beta = kwargs['beta_kmeans']
        self.threshold = kwargs['threshold']
        self.with_silence = kwargs['with_silence']
        self.nb_tries = kwargs['nb_tries']
        self.nb_steps = kwargs['nb_steps']

        # Negative Sampling for L41
        self.sampling = kwargs['sampling']
        self.ns_rate = kwargs['ns_rate']
        self.ns_method = kwargs['ns_method']

        self.add_dilated = kwargs['add_dilated']

        self.graph = get_default_graph()
        self.plugged = plugged
        # If the Separator is not independant but using a front layer (network.py:357-400)
        if self.plugged:
            self.F = kwargs['filters']
            g = self.graph
            self.training = g.get_tensor_by_name('inputs/is_training:0')
            front = g.get_tensor_by_name('front/output:0')
            non_mix_in = g.get_tensor_by_name('inputs/non_mix_input:0')
            self.x_non_mix = non_mix_in
            self.x_mix = g.get_tensor_by_name('inputs/mix_input:0')
            S, Fq = self.S, self.F

            with g.variable_scope('split_front'):
                def _x(run):
                    B = non_mix_in.value(run).shape[0]
                    return front.value(run)[:B]                          # [B, T, N] signed mixture representation
                self.X = Node('X', _x)
                x_split = self.X
                self.X_input = Node('X_input', lambda run: x_split.value(run))     # tf.identity(self.X), network.py:371

                def _xnm(run):
                    B = non_mix_in.value(run).shape[0]
                    return front.value(run)[B:]                          # rows (b,s): [B*S, T, N]
                self.X_non_mix_rows = Node('X_non_mix_rows', _xnm)
                self.X_non_mix = Node('X_non_mix', lambda run: self.X_non_mix_rows.value(run).reshape(
                    -1, S, self.X_non_mix_rows.value(run).shape[1], Fq).permute(0, 2, 3, 1))

            with g.variable_scope('create_masks'):
                def _y(run):
                    rows = self.X_non_mix_rows.value(run)
                    B = rows.shape[0] // S
                    # a DPCL training step feeds these labels to the fused loss: count them in the pass that writes them
                    weighted = self.function_mask in ('linear', 'sqrt', 'square') or self.loss_with_silence
                    E = getattr(self, 'count_labels_for', None) if (run.training and not weighted) else None
                    y = K.make_masks(rows, B, S, self.a, self.b, True, dpcl_E=E)  # [B, TF, S]
                    return self._weight_masks(y, run).reshape(B, rows.shape[1], Fq, S)
                self.y = Node('y', _y)

            self.I = g.get_tensor_by_name('inputs/indicies:0')
        else:
            # STFT hyperparams
            self.window_size = kwargs['window_size']
            self.hop_size = kwargs['hop_size']
            self.F = kwargs['window_size'] // 2 + 1
        # width of what the first BLSTM reads: the dilated stack (STFT path only; the front path ignores the flag, network.py:357-400)
        # leaves 4 channels per frequency
        self.in_dim = self.F * (4 if (self.add_dilated and not self.plugged) else 1)

    def _weight_masks(self, y, run):
        """network.py:381-396: magnitude-weighted masks / silence loss mask (off in the shipped launchers)."""
        if self.function_mask in ('linear', 'sqrt', 'square') or self.loss_with_silence:
            X = self.X.value(run)
            mode = self.function_mask if self.function_mask in ('linear', 'sqrt', 'square') else None
            y = K.weight_masks(X.contiguous(), y.contiguous(), mode,
                               self.threshold_silence_loss if self.loss_with_silence else None)
        return y

    def init_separator(self):
        if self.plugged:
            if self.abs_input:
                src = self.X
                self.X = Node('abs_input', lambda run: K.row_transform(src.value(run).contiguous(), pre='abs'), register=False)
            if self.normalize_input == '01':
                self.normalization01
            elif self.normalize_input == 'meanstd':
                self.normalization_mean_std
            self.prediction
        else:
            # STFT
            self.preprocessing
            if self.pre_func in ('sqrt', 'log'):
                src, fn = self.X, self.pre_func
                self.X = Node('pre_func', lambda run: K.row_transform(src.value(run).contiguous(), pre=fn), register=False)
            if self.normalize_input == '01':
                self.normalization01
            elif self.normalize_input == 'meanstd':
                self.normalization_mean_std
            if self.silent_threshold > 0:
                src, thr = self.X, self.silent_threshold

                def _sil(run):
                    return K.row_transform(src.value(run).contiguous(), norm='silent', thr=thr / 20.)
                self.X = Node('silent_mask', _sil, register=False)
            if self.add_dilated:
                self.dilated
            self.prediction
            if self.args['model_folder'] is None:
                self.cost_model = self.cost
                self.finish_construction()
                self.optimize

    def add_enhance_layer(self):
        self.separate
        self.enhance
        self.cost_model = self.enhance_cost
        self.finish_construction()
        self.freeze_all_except('enhance')
        self.optimize

    def add_finetuning(self):
        self.separate
        self.enhance
        self.postprocessing
        self.cost_finetuning
        self.cost_model = self.cost_finetuning
        self.finish_construction()
        to_train = []
        for var in self.trainable_variables:
            for p in self.args['train']:
                if p in var.ams_name:
                    to_train.append(var)
        self.trainable_variables = to_train
        self.optimize

    @scope
    def preprocessing(self):
        from ams_hip import stft_host
        return stft_host.build_preprocessing(self)

    @scope
    def normalization01(self):
        src = self.X

        def _n(run):
            return K.row_transform(src.value(run).contiguous(), norm='01')
        self.X = Node('X01', _n)
        return self.X

    @scope
    def normalization_mean_std(self):
        src = self.X

        def _n(run):
            return K.row_transform(src.value(run).contiguous(), norm='meanstd')
        self.X = Node('Xms', _n)
        return self.X

    @scope
    def prediction(self):
        pass

    @scope
    def dilated(self):
        """network.py:527-551: 13 dilated conv2d + ReLU layers over the conditioned magnitudes X [B,T,F] (NHWC, one channel) ->
        X [B,T,4F].  X_input, the magnitude `separate` masks, is not touched.  The reference reshapes to size_t from chunk_size, which
        is the STFT frame count for chunk-length inputs: the actual T is used."""
        specs = [((1, 7), (1, 1), 128), ((7, 1), (1, 1), 128)] + [((5, 5), (r, 1), 128) for r in (4, 8, 16, 32)] + \
                [((5, 5), (r, r), 128) for r in (1, 2, 4, 8, 16, 32)] + [((5, 5), (1, 1), 4)]
        layers, cin = [], 1
        for i, (kernel, rate, cout) in enumerate(specs):
            layers.append(Conv2D(cin, cout, kernel, rate, name='Conv' if i == 0 else 'Conv_%d' % i))
            cin = cout
        self.dilated_layers = layers
        src = self.X
        self.X = Node('output', lambda run: conv2d_stack(layers, src.value(run)))
        return self.X

    @scope
    def separate(self):
        from ams_hip import separate_host
        return separate_host.build_separate(self, KMeans)

    @scope
    def postprocessing(self):
        from ams_hip import stft_host
        return stft_host.build_postprocessing(self)

    @scope
    def enhance(self):
        from ams_hip import separate_host
        return separate_host.build_enhance(self, BLSTM, Conv1D, f_props)

    @scope
    def enhance_cost(self):
        from ams_hip import separate_host
        return separate_host.build_enhance_cost(self)

    @scope
    def cost_finetuning(self):
        from ams_hip import separate_host
        return separate_host.build_cost_finetuning(self, self.postprocessing)
