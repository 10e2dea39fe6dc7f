"""CPU: the site policy of the fused and the multi-head route (kgwas_amd.model.LayerSite, HeteroGNN._layer_site): which stages
follow the transform of layer l, which launch writes the next layer's row blocks, who applies the ReLU and who masks its gradient
-- for every combination of gnn_root_weight x gnn_norm x hidden dropout, L = 2 and 3, every layer, both ``last_premasked`` and both
modes, against the rule written out below as literal values.  No kernel is launched."""
import itertools

import pytest

# Layers BEFORE the last, by (root, norm, drop) -- drop: the model has gnn_dropout AND is in training mode:
# (the launch that gets the next layer's blocks; the transform's premasked, relu; the root's premasked, relu -- None without a
#  root; whether 'mean' carries the layer input on)
INNER = {
    (False, False, False): ('transform', True, True, None, None, False),
    (False, False, True): ('drop', True, True, None, None, True),
    (False, True, False): ('norm', True, False, None, None, True),
    (False, True, True): ('drop', True, False, None, None, True),
    (True, False, False): ('root', True, False, True, True, True),
    (True, False, True): ('drop', True, False, True, True, True),
    (True, True, False): ('norm', True, False, True, False, True),
    (True, True, True): ('drop', True, False, True, False, True),
}
# The LAST layer (no norm, no dropout behind it), by (root, last_premasked): the same fields
LAST = {
    (False, False): ('transform', False, True, None, None, False),
    (False, True): ('transform', True, True, None, None, False),
    (True, False): ('root', True, False, False, True, True),
    (True, True): ('root', True, False, True, True, True),
}
X_PREMASKED = {1: False, 2: True, 3: True}            # the root's input is a premasked producer's ReLU output from layer 2 on


@pytest.fixture(scope='module')
def tiny(tmp_path_factory):
    from kgwas_amd.kgwas_data import KGWAS_Data
    return KGWAS_Data.from_synthetic(scale=0.002, seed=3, feat_dims={'Gene': 40}, data_path=str(tmp_path_factory.mktemp('site')))


@pytest.mark.parametrize('layers', [2, 3])
@pytest.mark.parametrize('root,norm,dropout', list(itertools.product([False, True], repeat=3)))
def test_the_site_of_every_layer(tiny, layers, root, norm, dropout):
    from kgwas_amd.model import HeteroGNN
    dims = (tiny.snp_init_dim_size, tiny.gene_init_dim_size, tiny.go_init_dim_size)
    model = HeteroGNN(tiny.data, 128, 1, layers, 'GAT', 'sum', *dims, 1, gnn_root_weight=root, gnn_norm='layer' if norm else None,
                      gnn_dropout=0.3 if dropout else 0.0)
    n = 0
    for training, last_premasked, l in itertools.product([True, False], [False, True], range(1, layers + 1)):
        model.train(training)
        hdrop = model._hidden_dropout()
        assert (hdrop is not None) == (dropout and training)
        site = model._layer_site(l, hdrop, last_premasked)
        what = (layers, root, norm, dropout, training, last_premasked, l)
        if l < layers:
            writer, premasked, relu, r_premasked, r_relu, carried = INNER[(root, norm, dropout and training)]
        else:
            writer, premasked, relu, r_premasked, r_relu, carried = LAST[(root, last_premasked)]
        assert site.layer == l and site.writer == writer, what
        assert (site.premasked, site.relu) == (premasked, relu), what
        # the stages there are, and what they are given
        assert (site.root is not None) == root and (site.norm is not None) == (norm and l < layers), what
        assert (site.drop is not None) == (dropout and training and l < layers), what
        if root:
            assert site.root is model.root_weight[l - 1], what
            assert (site.root_premasked, site.root_relu, site.x_premasked) == (r_premasked, r_relu, X_PREMASKED[l]), what
        if site.norm is not None:
            assert site.norm[0] is model.norm_weight[l - 1] and site.norm[1] is model.norm_bias[l - 1], what
            assert site.norm_premasked is True, what
        if site.drop is not None:
            assert site.drop[0] == 0.3 and site.drop[1] is model.drop_word, what
        # exactly one stage, the last one present, receives the next layer's blocks
        nxt = ['blocks']
        got = {s: site.out_blocks(s, nxt) for s in ('transform', 'root', 'norm', 'drop')}
        assert got == {s: (nxt if s == writer else None) for s in got}, what
        present = ['transform'] + [s for s, on in (('root', site.root), ('norm', site.norm), ('drop', site.drop)) if on is not None]
        assert writer == present[-1], what
        # under 'mean' the scaled outputs are not the transform's blocks: the layer input is carried on only when a later launch
        # writes them
        assert (site.hbuf_after_mean('hbuf') == 'hbuf') == carried and site.hbuf_after_mean('hbuf') in ('hbuf', None), what
        n += 1
    assert n == 4 * layers
