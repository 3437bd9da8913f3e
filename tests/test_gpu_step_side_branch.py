"""GPU: the forward side branch of a training step (ams_hip/functional.py: FORWARD_BRANCH) -- the weight images of the layers above the
first and the labels with their counts, issued beside the first two layers' forward recurrences -- against the same step with everything
in line (AMS_FWD_BRANCH=0) and with one launch per image (AMS_PS_PACK_MANY=0).  Nothing but WHERE and in HOW MANY launches the images and
labels are made differs, so every cost and every updated variable must be bit-identical.

The switches are read once per process: one child process per setting, each training the smallest front_DPCL model of the step tests
(tests/smoke_step.py; its dX products are too narrow for the image form, so its branch carries W^T images and labels) and a wider
three-layer one (layer size 256: all six weight images), eager and captured (--hip_graph), in each of the two forward forms with the
form fixed: the autotuner's choice between them is a matter of timing, and the two forms are not the same bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import gc, os, sys, tempfile
import numpy as np
root = os.environ['AMS_ROOT']
sys.path[:0] = [root, os.path.join(root, 'adaptive-multispeaker-separation_amd')]
import torch
from ams_hip import functional as F, ops as K
from tests.smoke_step import build_front_dpcl
import utils.ops
out = {}
# The forward form is FIXED per run (no autotuner): a captured step otherwise measures both forms and keeps the faster one, the two forms
# differ in the order of their k-tiles, and which one a tiny model's timing picks is noise -- three processes would not agree on it.
K.PS_AUTOTUNE = False
gc.disable()
for tag, cfg in (('small', dict(layer_size=16, nb_layers=2)), ('wide', dict(layer_size=256, nb_layers=3))):
    for form in (1, 0):                                          # forward products from pre-split images / cut inside the product
        for graph in (False, True):
            K.PRESPLIT = bool(form) and K.F16X3
            utils.ops.rng.seed(42)
            torch.manual_seed(0)
            np.random.seed(0)
            f0, i0, p0 = F.FORWARD_BRANCH.fired, F.FORWARD_BRANCH.images, K.PS_LAUNCHES[0]
            trainer, tfds = build_front_dpcl(tempfile.mkdtemp(prefix='ams_sb_'), B=3, L=1024, W=64, N=16, hop=16, E=8, hip_graph=graph,
                                             no_summaries=True, **cfg)
            g, model = trainer.graph, trainer.model
            steps = 5 if graph else 3                            # captured: two eager steps, the capture, replays
            costs = []
            with g.as_default():
                feed = {tfds.handle: tfds.get_handle(tfds.TRAIN), tfds.chunk_size: 1024}
                tfds.initialize(tfds.TRAIN)
                for i in range(steps):
                    costs.append(np.float32(float(model.train(feed, i))))
            torch.cuda.synchronize()
            K.raise_on_ring_errors()
            k = '%s_%d_%d' % (tag, form, int(graph))
            out['cost_' + k] = np.array(costs, np.float32)
            for v in model.trainable_variables:
                out['var_%s_%s' % (k, v.ams_name.replace('/', '.'))] = v.detach().cpu().numpy()
            out['fired_' + k] = np.array([F.FORWARD_BRANCH.fired - f0, F.FORWARD_BRANCH.images - i0, K.PS_LAUNCHES[0] - p0])
            # a captured graph of THIS configuration must not be destroyed while the next one is capturing (the destructor of a graph
            # is refused during a capture and ends the process): drop it now, outside any capture, and keep the collector out of the steps
            del trainer, tfds, g, model
            gc.collect()
            torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
'''

SETTINGS = {'branch': dict(AMS_FWD_BRANCH='1', AMS_PS_PACK_MANY='1'), 'branch_single_launches': dict(AMS_FWD_BRANCH='1', AMS_PS_PACK_MANY='0'),
            'in_line': dict(AMS_FWD_BRANCH='0', AMS_PS_PACK_MANY='1')}


@pytest.fixture(scope='module')
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('side_branch')
    script = tmp / 'child.py'
    script.write_text(_CHILD)
    res = {}
    for name, env in SETTINGS.items():
        out = tmp / (name + '.npz')
        e = dict(os.environ, AMS_ROOT=ROOT, AMS_LOG_DIR=str(tmp / 'log'), **env)
        subprocess.run([sys.executable, str(script), str(out)], check=True, env=e, timeout=600)
        res[name] = dict(np.load(out))
    return res


@pytest.mark.parametrize('other', ['branch_single_launches', 'in_line'])
def test_costs_and_variables_are_bit_identical(runs, other):
    a, b = runs['branch'], runs[other]
    assert sorted(a) == sorted(b)
    keys = [k for k in a if k.startswith(('cost_', 'var_'))]
    assert len([k for k in keys if k.startswith('cost_')]) == 8 and len(keys) > 8 + 8 * 8
    bad = []
    for k in keys:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.all(np.isfinite(a[k])), k
        if a[k].tobytes() != b[k].tobytes():
            bad.append((k, float(np.abs(a[k].astype(np.float64) - b[k]).max()), float(np.abs(b[k]).max())))
    print('side branch against %s: %d arrays, not bit-identical (name, max |delta|, max |value|): %r' % (other, len(keys), bad))
    assert not bad
    for k in [k for k in keys if k.startswith('cost_')]:
        assert len(set(a[k].tolist())) > 2, k                   # the steps moved


def test_the_branch_ran_where_it_is_on_and_only_there(runs):
    for tag in ('small', 'wide'):
        for form in (1, 0):
            for graph in (0, 1):
                k = 'fired_%s_%d_%d' % (tag, form, graph)
                # passes: eager one per step; captured two eager steps and the capture.  Two branches per pass: beside the first ring the
                # images of the layers above and the labels, beside the second the dense layer's images
                fired, images, ps_launches = (int(v) for v in runs['branch'][k])
                passes = 3
                assert fired == 2 * passes, (k, fired)
                assert (ps_launches > 0) == bool(form), (k, ps_launches)          # the run took the forward form it was told to
                # the pre-split form: at least the W^T images of the layer above and of the dense layer; the in-product form carries the dX
                # images only, which the small model's products are too narrow for
                # (first pass, later passes): the layers' dX images are cut once their gradient views exist
                first, later = {('small', 1): (2, 2), ('small', 0): (0, 0), ('wide', 1): (3, 3), ('wide', 0): (1, 3)}[(tag, form)]
                assert images >= first + (passes - 1) * later and (later or images == 0), (k, images)
                assert tuple(runs['branch_single_launches'][k]) == tuple(runs['branch'][k])
                assert tuple(runs['in_line'][k][:2]) == (0, 0) and (int(runs['in_line'][k][2]) > 0) == bool(form)


def test_frozen_owners_keep_their_images():
    """ops.cut_weight_images keeps ops.derived's rule: an image cut in this pass, or whose owners are all frozen, is valid -- its region is
    left out and the stored tensor stays; anything else is cut again in the next pass."""
    from ams_hip import ops as K
    rng = np.random.RandomState(5)
    W = torch.from_numpy(rng.uniform(-1, 1, (256, 512)).astype(np.float32)).cuda()
    V = torch.from_numpy(rng.uniform(-1, 1, (256, 512)).astype(np.float32)).cuda()
    bound = torch.ones(1, device='cuda')
    M = 192
    req = lambda t: ([(M, t, bound, (t,), '')], [(M, t, bound, (t,), '')])
    K.set_frozen(W, True)
    try:
        K.PASS[0] += 1
        assert K.cut_weight_images(*req(W)) == 2 and K.cut_weight_images(*req(V)) == 2
        kept = {n: K.derived_entry(W, n)[0] for n in ('ps_w', 'ps_dx')}
        first = {n: K.derived_entry(V, n)[0] for n in ('ps_w', 'ps_dx')}
        assert torch.equal(kept['ps_w'], K.ps_pack_cols(W, bound)) and torch.equal(kept['ps_dx'], K.ps_pack_rows(W, bound))
        assert K.cut_weight_images(*req(W)) == 0 and K.cut_weight_images(*req(V)) == 0      # the same pass: both valid
        K.PASS[0] += 1
        before = {n: kept[n].clone() for n in kept}
        assert K.cut_weight_images(*req(W)) == 0                 # frozen: kept across passes, nothing launched, same tensors
        assert K.cut_weight_images(*req(V)) == 2                 # live weights: cut again
        for n in kept:
            assert K.derived_entry(W, n)[0] is kept[n] and torch.equal(kept[n], before[n])
            assert K.derived_entry(V, n)[0] is not first[n]
        # the consumers find what the branch stored
        assert K._ps_weight_image(V, bound, (V,)) is K.derived_entry(V, 'ps_w')[0]
        assert K._ps_dx_weight_image(V, bound, (V,)) is K.derived_entry(V, 'ps_dx')[0]
    finally:
        K.set_frozen(W, False)
