# -*- coding: utf-8 -*-
"""DANet-SCE separator (reference models/SC_V2.py), host mirror over the HIP kernels: the source-contrastive cost of L41Model on
l2-normalised embeddings plus a deep-attractor reconstruction cost whose attractors are the ideal-mask means of the embeddings."""
import numpy as np

from ams_hip import functional as F
from ams_hip import ops as K
from ams_hip.graph import Node, get_default_graph, scope
from models.network import Separator
from utils.ops import BLSTM, Conv1D, f_props, _graph_rng


class L41ModelV2(Separator):

    def __init__(self, graph=None, **kwargs):
        kwargs['mask_a'] = 1.0
        kwargs['mask_b'] = -1.0

        if kwargs.get('nb_speakers', 0) > 4:
            # the attractor / reconstruction kernels (csrc/danet.hip) keep one float4 of masks per bin: four speakers
            raise ValueError('--nb_speakers %d: L41ModelV2 (DANet-SCE) supports at most 4 speakers -- its attractor and reconstruction '
                             'kernels hold four masks per bin; the other separators take up to 6' % kwargs['nb_speakers'])

        super(L41ModelV2, self).__init__(graph, **kwargs)
        K.check_danet_domain(self.embedding_size, self.S)       # the source-contrastive term's table (ops.check_l41_domain) contains it

        if self.loss_with_silence and self.add_dilated and not self.plugged:
            # SC_V2.py:51-56: the mask is taken from the X the prediction reads -- [B,T,4F] behind the dilated stack -- and multiplied
            # onto a [B,T,F,S] y: the reference's graph does not build for this pair either
            raise ValueError('--add_dilated --silence_loss: L41ModelV2 takes its silence mask from the input of the BLSTM stack, which is '
                             '[B, T, 4F] behind the dilated convolutions and cannot weight the [B, T, F, S] masks')

        # Define the speaker vectors to use during training (SC_V2.py:16-18): truncated normal, stddev sqrt(2/E)
        E = self.embedding_size

        def _trunc_normal(shape):
            sd = np.sqrt(2.0 / float(E))
            r = _graph_rng()
            v = r.standard_normal(shape) * sd
            bad = np.abs(v) > 2 * sd
            while bad.any():                                   # tf.truncated_normal re-draws beyond 2 sigma
                v[bad] = r.standard_normal(int(bad.sum())) * sd
                bad = np.abs(v) > 2 * sd
            return v.astype('float32')
        self.speaker_vectors = get_default_graph().get_variable('speaker_centroids', (self.num_speakers, E), _trunc_normal)
        self.init_separator()

    @scope
    def prediction(self):
        # SC_V2.py:21-42: BLSTM x nb_layers -> Conv1D -> [B,T,F,E]; NO Normalize layer, whatever --no_normalize says
        E, Fq = self.embedding_size, self.F
        y = self.y
        self.true_masks = Node('true_masks', lambda run: 1.0 + y.value(run), register=False)
        layers = [BLSTM(self.layer_size, name='BLSTM_' + str(i), drop_val=self.rdropout,
                        in_dim=(self.in_dim if i == 0 else self.layer_size)) for i in range(self.nb_layers)]
        conv = Conv1D([1, self.layer_size, E * Fq])
        x_node = self.X

        self._embed = Node('embed', lambda run: conv.f_prop(f_props(layers, x_node.value(run), then=conv)), register=False)
        self._embed_normalized = False                      # `separate` hands the prediction itself to k-means (which normalises its input)
        embed = self._embed

        def _pred(run):
            u = embed.value(run)
            return u.reshape(u.shape[:-1] + (Fq, E))
        return Node('prediction', _pred, register=False)

    @scope
    def cost(self):
        # SC_V2.py:44-127: sc_cost (l2-normalised embeddings and speaker vectors, always; no negative sampling) + cost_recons
        embed, y, I, spk = self._embed, self.y, self.I, self.speaker_vectors
        X, X_input, X_non_mix = self.X, self.X_input, self.X_non_mix
        thr = self.threshold_silence_loss if self.loss_with_silence else None

        def _both(run):
            yv = y.value(run)
            B, S = yv.shape[0], yv.shape[-1]
            xs = y_ab = None
            if thr is not None:
                # :50-56: mask = log10(max|X| / |X|) < threshold from the X the prediction reads; y_ab = y mask here, m = (y+1)/2 mask
                # inside the attractor pass
                xs = X.value(run).contiguous()
                y_ab = K.weight_masks(xs.reshape(B, -1), yv.reshape(B, -1, S).contiguous(), None, thr)
            return F.danet_sce_loss(embed.value(run), yv if y_ab is None else y_ab, yv, spk, I.value(run), X_input.value(run),
                                    X_non_mix.value(run), xs, thr)
        both = Node('cost_terms', _both, register=False)
        cost = Node('cost_value', lambda run: both.value(run)[0])
        s = get_default_graph().summaries                      # SC_V2.py:92,122,125 inside the 'cost' scope
        s['cost/reconstruction_loss/value'] = Node('reconstruction_loss/value', lambda run: both.value(run)[2])
        s['cost/source_contrastive_loss/value'] = Node('source_contrastive_loss/value', lambda run: both.value(run)[1])
        s['cost/total'] = Node('total', lambda run: both.value(run)[0])
        s['cost/cost'] = cost
        return cost
