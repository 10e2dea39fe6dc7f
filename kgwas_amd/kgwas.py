"""``KGWAS`` trainer -- the reference's driver API (kgwas/kgwas.py:25-212) on the MI355X path.

Kept verbatim from the reference: constructor / ``initialize_model`` / ``train`` / ``load_pretrained``
signatures and defaults, the attributes they set (``model``, ``best_model``, ``config``,
``train_loader`` ... ``infer_loader``, ``save_name``, ``kgwas_res``), the LD-weighted MSE
(kgwas.py:142-145), Adam(lr, weight_decay as L2) (kgwas.py:116), best-model selection by validation
Pearson (kgwas.py:170-173), checkpoint files (utils.py:203-207).

Deliberately different (Appendix A of SURVEY.md): no CUDA_LAUNCH_BLOCKING, no per-seed ``.item()``
dict look-ups (LD weights are a resident float64 vector indexed by SNP id), evaluation under no_grad.
Multi-GPU: one process per GPU (torch.distributed, RCCL); every rank trains on its own slice of each
batch and parameter gradients are all-reduced in one flat bucket (kgwas_amd/dist.py).
"""
from __future__ import annotations

import os
import pickle
from copy import deepcopy

import numpy as np
import torch
import torch.nn.functional as F

from . import dist as kdist
from . import ops
from .model import HeteroGNN
from .sampler import NeighborLoader, dropout_word
from .utils import (compute_metrics, evaluate_minibatch_clean, get_network_weight, load_pretrained, print_sys, write_tsv,
                    save_model)


class KGWAS:
    def __init__(self, data, weight_bias_track=False, device='cuda', proj_name='KGWAS', exp_name='KGWAS',
                 seed=42):
        torch.manual_seed(seed)                                     # kgwas.py:33-35
        if torch.cuda.is_available():
            torch.cuda.manual_seed(seed)
        np.random.seed(seed)
        self.seed = seed
        self.device = device if torch.cuda.is_available() else 'cpu'
        self.data = data
        self.data_path = data.data_path
        if weight_bias_track:
            import wandb
            wandb.init(project=proj_name, name=exp_name)
            self.wandb = wandb
        else:
            self.wandb = False
        self.exp_name = exp_name

    def initialize_model(self, gnn_num_layers=2, gnn_hidden_dim=128, gnn_backbone='GAT', gnn_aggr='sum',
                         gat_num_head=1, no_relu=False, out_channels=1, gat_dropout=0.0, gat_sigmoid=False, gat_temperature=1.0,
                         gat_edge_dim=None, gnn_dropout=0.0, gnn_norm=None, gnn_root_weight=False):
        """``out_channels`` (extra, default 1 = the reference, kgwas.py:52): T > 1 reads ONE shared trunk out into T label columns
        (``data['SNP'].y`` [N, T], KGWAS_Data.from_synthetic(n_traits=T)) -- a shared-trunk multi-task model, not T independent
        models.  It enters ``config`` only when it is not 1, so the config.pkl of a single-trait run is what it always was.
        ``gat_dropout`` (extra, default 0 = the reference): attention dropout p of the GAT layers while training (HeteroGNN); it
        enters ``config`` only when it is not 0.
        ``gat_num_head`` = H in (2, 4): H attention heads of width gnn_hidden_dim / H, concatenated back to gnn_hidden_dim (PyG's
        GATConv(hidden // H, heads=H); HeteroGNN(gat_split_heads=True)) -- not the reference's literal widening to H * hidden.
        ``gat_sigmoid`` / ``gat_temperature`` (extras, defaults False / 1 = the reference's model; its GATConv's ``sigmoid_gat`` and
        ``temperature``, conv.py:49-50): sigmoid gates instead of the softmax, and the divisor T of the attention logits (HeteroGNN).
        Each enters ``config`` only when it is not the default.
        ``gat_edge_dim`` = D in 1..8 (extra, default None = the reference's model, launch for launch and bit for bit): GATConv's
        ``edge_dim`` (conv.py:46,207-215) for the relations whose ``data[edge_type].edge_attr`` is set (KGWAS_Data.set_edge_attr /
        from_synthetic(edge_dim=D)); it enters ``config`` only when it is set.  GAT only; not with gat_num_head > 1, gat_dropout > 0
        or gat_sigmoid; training takes whole neighbourhoods (no ``num_neighbors``) and parallelism='seed'.
        ``gnn_dropout`` (extra, default 0 = the reference): dropout p on the hidden state between the message-passing layers while
        training (HeteroGNN; needs gnn_num_layers >= 2); every backbone and switch takes it, parallelism='shard' does not.  It
        enters ``config`` only when it is not 0.
        ``gnn_norm`` = 'layer' (extra, default None = the reference's model, launch for launch and bit for bit): a learned LayerNorm
        per node type on the output of every message-passing layer but the last, before its ReLU (HeteroGNN; needs
        gnn_num_layers >= 2), in training, evaluation and the attention queries alike; every backbone and switch takes it,
        parallelism='shard' does not.  It enters ``config`` only when it is set.
        ``gnn_root_weight`` = True (extra, default False = the reference's model, launch for launch and bit for bit): a learned
        bias-free Linear per layer and node type on every destination node's OWN layer input, added to the relation sum / mean /
        min / max before the norm and the ReLU (HeteroGNN) -- the self term the reference's GATConv(add_self_loops=False) relations
        leave out -- in training, evaluation and the attention queries alike; GAT with every switch takes it, gnn_backbone='SAGE'
        (whose lin_r already is one) and parallelism='shard' do not.  It enters ``config`` only when it is True."""
        if gnn_root_weight and gnn_backbone == 'SAGE':
            raise ValueError("gnn_root_weight needs gnn_backbone='GAT': SAGE's lin_r already is a root weight per relation")
        if gnn_norm not in (None, 'layer'):
            raise ValueError(f"gnn_norm {gnn_norm!r}: None or 'layer'")
        if gnn_norm is not None and int(gnn_num_layers) < 2:
            raise ValueError(f'gnn_norm needs gnn_num_layers >= 2 (got {gnn_num_layers}): the norm sits between the layers')
        self.config = {'gnn_num_layers': gnn_num_layers, 'gnn_hidden_dim': gnn_hidden_dim,
                       'gnn_backbone': gnn_backbone, 'gnn_aggr': gnn_aggr, 'gat_num_head': gat_num_head}
        out_channels = int(out_channels)
        if not 1 <= out_channels <= 32:
            raise NotImplementedError(f'out_channels = {out_channels}: the read-out kernels take 1 to 32 label columns')
        if out_channels != 1:
            self.config['out_channels'] = out_channels
        gat_dropout = float(gat_dropout)
        if gat_dropout != 0.0:
            self.config['gat_dropout'] = gat_dropout
        gat_sigmoid, gat_temperature = bool(gat_sigmoid), float(gat_temperature)
        if gat_sigmoid:
            self.config['gat_sigmoid'] = True
        if gat_temperature != 1.0:
            self.config['gat_temperature'] = gat_temperature
        if gat_edge_dim is not None:
            self.config['gat_edge_dim'] = int(gat_edge_dim)
        gnn_dropout = float(gnn_dropout)
        if gnn_dropout != 0.0:
            self.config['gnn_dropout'] = gnn_dropout
        if gnn_norm is not None:
            self.config['gnn_norm'] = gnn_norm
        if gnn_root_weight:
            self.config['gnn_root_weight'] = True
        self.gnn_num_layers = gnn_num_layers
        self.model = HeteroGNN(self.data.data, gnn_hidden_dim, out_channels, gnn_num_layers, gnn_backbone, gnn_aggr,
                               self.data.snp_init_dim_size, self.data.gene_init_dim_size,
                               self.data.go_init_dim_size, gat_num_head, no_relu=no_relu, gat_dropout=gat_dropout,
                               gat_split_heads=True, gat_sigmoid=gat_sigmoid, gat_temperature=gat_temperature,
                               gat_edge_dim=gat_edge_dim, gnn_dropout=gnn_dropout, gnn_norm=gnn_norm,
                               gnn_root_weight=bool(gnn_root_weight)).to(self.device)

    def load_pretrained(self, path):
        import pandas as pd
        with open(os.path.join(path, 'config.pkl'), 'rb') as f:
            config = pickle.load(f)
        self.initialize_model(**config)
        self.config = config
        self.model = load_pretrained(path, self.model).to(self.device)
        self.best_model = self.model
        pred_csv = os.path.join(path, 'pred.csv')
        if os.path.exists(pred_csv):
            self.kgwas_res = pd.read_csv(pred_csv, sep=None, engine='python')
        self.save_name = path.split('/')[-1]

    # ------------------------------------------------------------------------------------------
    def _ld_weight_vector(self) -> torch.Tensor:
        """float64 [N_SNP] LD-score regression weight per SNP index (kgwas.py:142-143 without the
        per-step Python look-ups); SNPs without a weight get 0 and are never seeds.  A data object with per-trait weights
        (``ldsc_weight_traits``, KGWAS_Data.from_synthetic(trait_sample_sizes=) / load_external_gwas_traits) gives [N_SNP, T]: one
        weight per (SNP, trait), 0 where the trait is not observed -- the read-out node's kgw_readout_wmse_mtw_* form."""
        n = int(self.data.data['SNP'].x.shape[0])
        wt = getattr(self.data, 'ldsc_weight_traits', None)
        if wt is not None:
            wt = np.ascontiguousarray(wt, dtype=np.float64)
            w = torch.zeros(n, wt.shape[1], dtype=torch.float64)
            w[torch.from_numpy(np.asarray(self.data.all_ids, dtype=np.int64))] = torch.from_numpy(wt)
            return w.to(self.device)
        w = torch.zeros(n, dtype=torch.float64)
        ids = np.asarray(self.data.all_ids, dtype=np.int64)
        w[torch.from_numpy(ids)] = torch.from_numpy(np.asarray(self.data.ldsc_weight, dtype=np.float64))
        return w.to(self.device)

    def make_loaders(self, batch_size, num_workers=0, num_neighbors=None, epoch_order='fixed'):
        """``num_neighbors`` (extra, None = the reference's [-1] * L): fan-outs of the TRAINING loader only; validation, test
        and inference always take full neighbourhoods, as the reference does.  ``epoch_order`` (extra, 'fixed' = the reference):
        the per-epoch order of the TRAINING loader's seeds (NeighborLoader); the other loaders keep the order given."""
        kwargs = {'batch_size': batch_size, 'num_workers': num_workers, 'drop_last': True, 'device': self.device}
        eval_kwargs = {'batch_size': 512, 'num_workers': num_workers, 'drop_last': False, 'device': self.device}
        L = self.gnn_num_layers
        rank, world = kdist.rank_world()
        tr_type, tr_ids = self.data.train_input_nodes
        if epoch_order == 'fixed':
            tr_ids = kdist.shard_batches(np.asarray(tr_ids), batch_size, rank, world)
            tr_kwargs = dict(kwargs, batch_size=batch_size // world)      # each rank: its slice of every batch
        else:                                                             # (a shuffled order: the loader slices the epoch's order)
            if batch_size % world:
                raise ValueError(f'batch_size {batch_size} must be divisible by world size {world}')
            tr_kwargs = dict(kwargs, batch_size=batch_size // world, epoch_order=epoch_order, rank=rank, world=world)
        self.train_loader = NeighborLoader(self.data.data, num_neighbors=[-1] * L if num_neighbors is None else num_neighbors,
                                           sampler=None, input_nodes=(tr_type, tr_ids), seed=self.seed, **tr_kwargs)        # kgwas.py:99-101
        self.val_loader = NeighborLoader(self.data.data, num_neighbors=[-1] * L,
                                         input_nodes=self.data.val_input_nodes, **kwargs)     # :102-103
        self.test_loader = NeighborLoader(self.data.data, num_neighbors=[-1] * L,
                                          input_nodes=self.data.test_input_nodes, **eval_kwargs)  # :104-105
        infer_idx = np.asarray(self.data.all_ids)                                             # :107-110
        self.infer_loader = NeighborLoader(self.data.data, num_neighbors=[-1] * L,
                                           input_nodes=('SNP', infer_idx), **eval_kwargs)     # :112-113

    def train_step(self, batch, optimizer, ld_w, world: int = 1, loss_rule=None):
        """kgwas.py:130-151 for one batch; returns the (float64) loss tensor, no host sync.  ``loss_rule`` (optim.parse_loss; None =
        the reference's weighted MSE): the read-out node's loss."""
        optimizer.zero_grad(set_to_none=True)
        bs = batch['SNP'].batch_size
        # forward + mean(ld_weight * (pred - y)**2) in float64 (kgwas.py:137-145); labels / weights by the seeds' ids
        loss, _ = self.model.forward_loss(batch.x_dict, batch.edge_index_dict, bs, batch.n_id('SNP'), batch.dg.y['SNP'], ld_w,
                                          unit_grad=True, loss_rule=loss_rule)
        loss.backward(gradient=ops.unit_gradient(loss.device))      # (the resident 1.0: no ones_like fill, see readout_weighted_mse)
        if world > 1:
            kdist.allreduce_grads(self.model, world)
        optimizer.step()
        return loss

    def _train_sharded(self, batch_size, lr, weight_decay, total_epoch, save_best_model, save_name, use_graph=True,
                       lr_schedule=None, grad_clip_norm=None, weight_average=None, loss=None):
        """kgwas/kgwas.py:85-212 in the SNP-sharded multi-GPU mode (kgwas_amd/shard.py): every rank works on the SAME
        batches of the reference's order and owns the SNPs of one id range; validation / test / inference predictions are
        computed shard-wise and summed, so every rank sees the same metrics and keeps the same best model."""
        from .shard import ShardedTrainer
        if lr_schedule is not None or grad_clip_norm is not None:
            raise NotImplementedError("lr_schedule / grad_clip_norm are not available with parallelism='shard': the sharded step "
                                      "calls the optimiser without its controls; use parallelism='seed'")
        if weight_average is not None:
            raise NotImplementedError("weight_average is not available with parallelism='shard': the sharded step does not run "
                                      "the weight-averaging launch; use parallelism='seed'")
        if loss is not None:
            raise NotImplementedError("loss is not available with parallelism='shard': the sharded step has its own read-out and "
                                      "loss; use parallelism='seed'")
        if getattr(self.model, 'heads', 1) > 1:
            raise NotImplementedError("gat_num_head > 1 is not available with parallelism='shard': the partial softmax states of "
                                      "the SNP-sharded exchange are single-head; use parallelism='seed'")
        if getattr(self.model, 'gat_dropout', 0.0) > 0:
            raise NotImplementedError("gat_dropout > 0 is not available with parallelism='shard': it would drop inside partial "
                                      "softmax states; use parallelism='seed'")
        if getattr(self.model, 'gnn_dropout', 0.0) > 0:
            raise NotImplementedError("gnn_dropout > 0 is not available with parallelism='shard': the sharded step does not run "
                                      "the hidden-state dropout launches; use parallelism='seed'")
        if getattr(self.model, 'gnn_norm', None) is not None:
            raise NotImplementedError("gnn_norm is not available with parallelism='shard': the sharded step does not run the "
                                      "layer-normalisation launches; use parallelism='seed'")
        if getattr(self.model, 'gnn_root_weight', False):
            raise NotImplementedError("gnn_root_weight is not available with parallelism='shard': the sharded step does not run the "
                                      "root-weight launches; use parallelism='seed'")
        if getattr(self.model, 'gat_sigmoid', False) or getattr(self.model, 'temperature', 1.0) != 1.0:
            raise NotImplementedError("gat_sigmoid / gat_temperature are not available with parallelism='shard': the exchange of "
                                      "partial softmax states is built for the softmax at T = 1; use parallelism='seed'")
        if getattr(self.model, 'edge_dim', None) is not None:
            raise NotImplementedError("gat_edge_dim is not available with parallelism='shard': the edge-attribute forward does not "
                                      "leave partial softmax states; use parallelism='seed'")
        if self.model.lin.out_features != 1:
            raise NotImplementedError("out_channels > 1 (multi-trait labels) is not available with parallelism='shard': the "
                                      "sharded step's read-out and loss are single-column; use parallelism='seed'")
        if getattr(self.data, 'ldsc_weight_traits', None) is not None:
            raise NotImplementedError("per-trait LD weights are not available with parallelism='shard'; use parallelism='seed'")
        rank, world = kdist.rank_world()
        if world > 1:
            kdist.broadcast_params(self.model)
        st = ShardedTrainer(self, self.data.train_input_nodes, batch_size, lr=lr, weight_decay=weight_decay, use_graph=use_graph)
        y_all = self.data.data['SNP'].y

        def evaluate(ids, model, drop_last=False):
            ids = np.asarray(ids)
            if drop_last:                                   # the reference's val loader drops the partial batch (kgwas.py:102-103)
                ids = ids[:len(ids) // batch_size * batch_size]
            pred = st.predict(ids, model).cpu().numpy()
            return {'pred': pred, 'truth': y_all[torch.from_numpy(ids)].numpy()}

        min_val = -1000
        self.best_model = deepcopy(self.model).to(self.device)
        print_sys('Start Training (SNP-sharded over %d ranks)...' % world)
        for ep in range(total_epoch):
            self.model.train()
            for step in range(st.n_batches):
                st.step(step)
                if (step % 500 == 0) and (step >= 500):
                    print_sys('Epoch {} Step {} Train Loss (this rank\'s share): {:.4f}'.format(ep + 1, step + 1, float(st.last_loss)))
            st.check()                                      # (captured form: no batch overflowed the static layout)
            val_metrics = compute_metrics(evaluate(self.data.val_input_nodes[1], self.model, True), False, -1, -1, F.mse_loss)
            print_sys('Epoch {}: Validation MSE: {:.4f} Validation Pearson: {:.4f}. '.format(
                ep + 1, val_metrics['mse'], val_metrics['pearsonr']))
            self.val_metrics = val_metrics
            if val_metrics['pearsonr'] > min_val:                    # kgwas.py:170-173
                min_val = val_metrics['pearsonr']
                self.best_model = deepcopy(self.model)
        if save_best_model and rank == 0:
            save_model_path = os.path.join(self.data_path, 'model')
            save_model(self.best_model, self.config, os.path.join(save_model_path, save_name))
        self.test_metrics = compute_metrics(evaluate(self.data.test_input_nodes[1], self.best_model), False, -1, -1, F.mse_loss)
        self.data.lr_uni['pred'] = evaluate(self.data.all_ids, self.best_model)['pred']                  # kgwas.py:189-191
        self._postprocess(save_name, save_best_model and rank == 0)
        self.shard_bytes_moved = st.xchg.bytes_moved

    def train(self, batch_size=512, num_workers=0, lr=1e-4, weight_decay=5e-4, epoch=10, save_best_model=True,
              save_name=None, data_to_cuda=False, use_graph=True, parallelism='seed', num_neighbors=None, shuffle=False,
              lr_schedule=None, grad_clip_norm=None, weight_average=None, loss=None):
        """Same signature and defaults as kgwas/kgwas.py:85-87.  ``use_graph`` (extra, default on): run the
        training step as one captured HIP graph (kgwas_amd/graph_step.py); off = eager launches, same math.
        ``parallelism`` (extra; matters under torch.distributed): 'seed' = every rank trains on its slice of each batch
        against a replicated graph (kgwas_amd/dist.py); 'shard' = SNP rows sharded by id range, Gene / GO replicated
        (kgwas_amd/shard.py, BASELINE.json north_star).
        ``num_neighbors`` (extra, default None = the reference's [-1] * L): PyG's list form [k_1, ..., k_L] for the TRAINING
        loader -- at most k_h in-edges per (node, relation) at hop h, redrawn every epoch from (the run's seed, epoch, batch
        index); evaluation and inference keep full neighbourhoods.  Not available with parallelism='shard'.
        ``shuffle`` (extra, default False = the reference, which visits its training SNPs in genome order every epoch,
        kgwas/kgwas.py:93-94): True = every epoch visits the training seeds in an order of its own (what PyG's shuffle=True means;
        NeighborLoader(epoch_order='seeds')), 'batches' = the fixed order's genome-contiguous batches, visited in another order
        every epoch.  The order is a pure function of (the run's seed, epoch), the same on every rank.  An argument of the run,
        not of the model: nothing enters config.pkl.  Validation, test and inference keep their order.  Not available with
        parallelism='shard'.
        ``lr_schedule`` (extra, default None = the reference's one rate): a kind ('constant', 'linear', 'cosine', 'step') or a dict
        with ``kind``, ``warmup_steps``, ``min_lr``, ``step_size``, ``gamma``, ``total_steps`` (optim.parse_lr_schedule; the rule:
        include/kgwas_hip.h); ``total_steps`` defaults to ``epoch`` x the batches of an epoch.  The rate of every update is formed
        inside the optimiser's kernel from the device step counter.  ``grad_clip_norm`` (extra, default None): finite and > 0, the
        max_norm of torch.nn.utils.clip_grad_norm_ over all gradients, applied inside the update (the gradient tensors stay
        unscaled).  With either set the eager loop (``use_graph=False``) runs FusedAdam too -- both loops the same kernels -- and
        ``self.last_lr`` holds the rate of the epoch's last update, read at the validation point (wandb: ``lr``).  Arguments of the
        run: nothing enters config.pkl.  Not available with parallelism='shard'.
        ``weight_average`` (extra, default None = the reference, which evaluates, selects and saves the raw weights): 'ema' | 'swa' |
        a float (EMA with that decay) | a dict with ``kind``, ``decay`` (0.999), ``warmup`` (True), ``start_step`` (1), ``every``
        (1, or 'epoch') (optim.parse_weight_average; the rule: include/kgwas_hip.h, KgwWeightAvg).  ``self.avg_model`` is an averaged
        copy of the weights, moved on the device by one launch behind the optimiser's; ``self.model`` stays the raw model.  An epoch
        that ends after the first averaging event validates ``avg_model``, and ``best_model`` -- what test, inference and model.pt
        go through -- is a copy of it when its Pearson is the best so far; an epoch that ends before the first event does what the
        default run does.  The eager loop (``use_graph=False``) runs FusedAdam too: both loops the same kernels and the same
        counter.  An argument of the run: nothing enters config.pkl.  Not available with parallelism='shard'; with several ranks
        every rank applies the same update, so the shadows agree (run on one rank only so far).
        ``loss`` (extra, default None = the reference's LD-weighted MSE, kgwas/kgwas.py:139-145): 'mse' | 'huber' (delta 1.0) | a
        float (Huber with that delta) | a dict with ``kind`` and ``delta`` -- a float > 0 or one per label column (traits have their
        own scales); optim.parse_loss, the rule: include/kgwas_hip.h, KgwReadoutLossArgs.  The TRAINING loss becomes the weighted
        Huber loss 1/N sum w rho_delta(pred - y), rho = r^2 up to |r| = delta and delta (2 |r| - delta) beyond: a residual's pull
        on the gradient is bounded by 2 delta w / N, so the SNPs of a top locus no longer decide a batch.  It is computed inside the
        read-out node's own kernels (single trait, T traits, per-trait weights with unobserved pairs), so the captured step keeps its
        route, its launches and its fused optimiser launch, and the eager loop runs the same kernels.  delta = +inf is the MSE, to
        the bit.  Validation, test and model selection keep MSE / Pearson.  An argument of the run: nothing enters config.pkl.  Not
        available with parallelism='shard'; parallelism='seed' needs nothing new (run on one rank only so far)."""
        total_epoch = epoch
        from .optim import check_grad_clip_norm, parse_lr_schedule, parse_weight_average, parse_loss
        grad_clip_norm = check_grad_clip_norm(grad_clip_norm)
        loss_rule = parse_loss(loss, self.model.lin.out_features)    # (a ValueError before anything is built; 'mse' is the default route)
        controlled = lr_schedule is not None or grad_clip_norm is not None
        parse_weight_average(weight_average, 1)                      # (a ValueError before anything is built; 'epoch' is resolved below)
        if isinstance(shuffle, (bool, np.bool_)):
            epoch_order = 'seeds' if shuffle else 'fixed'
        elif isinstance(shuffle, str) and shuffle == 'batches':
            epoch_order = 'batches'
        else:
            raise ValueError(f"shuffle {shuffle!r}: False, True or 'batches'")
        if epoch_order != 'fixed' and parallelism == 'shard':
            raise NotImplementedError("shuffle is not available with parallelism='shard': the sharded trainer walks the fixed "
                                      "order's batches")
        if num_neighbors is not None:
            from .sampler import check_num_neighbors
            if not isinstance(num_neighbors, dict) and len(num_neighbors) != self.gnn_num_layers:
                raise ValueError(f'num_neighbors needs one entry per layer ({self.gnn_num_layers})')
            if check_num_neighbors(num_neighbors) is None:
                num_neighbors = None                                   # [-1] * L: the default path
            elif parallelism == 'shard':
                raise NotImplementedError("a finite fan-out is not available with parallelism='shard': the ranks would have "
                                          "to agree on the draw of every replicated row")
            elif getattr(self.model, 'edge_dim', None) is not None:
                raise NotImplementedError('gat_edge_dim with a finite num_neighbors: a drawn segment keeps no record of which '
                                          'entries of its row it holds, so its edges cannot find their attributes')
        if save_name is None:
            save_name = self.exp_name
        self.save_name = save_name
        if parallelism == 'shard':
            return self._train_sharded(batch_size, lr, weight_decay, total_epoch, save_best_model, save_name, use_graph,
                                       **({'lr_schedule': lr_schedule, 'grad_clip_norm': grad_clip_norm} if controlled else {}),
                                       **({'weight_average': weight_average} if weight_average is not None else {}),
                                       **({'loss': loss_rule} if loss_rule is not None else {}))
        if parallelism != 'seed':
            raise ValueError(f"parallelism {parallelism!r}: 'seed' or 'shard'")
        print_sys('Creating data loader...')
        self.make_loaders(batch_size, num_workers, num_neighbors, epoch_order)
        rank, world = kdist.rank_world()
        if world > 1:
            kdist.broadcast_params(self.model)
        controls = {}
        if controlled:
            if lr_schedule is not None:
                lr_schedule = parse_lr_schedule(lr_schedule, lr, max(1, total_epoch * len(self.train_loader)))
            controls = {'lr_schedule': lr_schedule, 'grad_clip_norm': grad_clip_norm}
        weight_average = parse_weight_average(weight_average, max(1, len(self.train_loader)))
        if weight_average is not None:
            controls['weight_average'] = weight_average
        graph_step = wavg = None
        if use_graph and len(self.train_loader) > 0:
            from .graph_step import GraphTrainStep
            # (multi-GPU: a 512-seed batch split over the ranks = strong scaling; from 4 ranks on the batch-independent first gene
            #  Linear is split by gene rows instead of repeated on every rank -- ops.GeneLayerShard)
            shuffled = {} if epoch_order == 'fixed' else {'epoch_order': epoch_order, 'epochs': total_epoch, 'rank': rank, 'world': world}
            graph_step = GraphTrainStep(self, (self.train_loader.input_type, self.train_loader.ids.cpu().numpy()),
                                        self.train_loader.batch_size, lr=lr, weight_decay=weight_decay,
                                        shard_gene_layer=None, **shuffled, **controls, loss=loss_rule,
                                        # (the loader's batch order is fixed, kgwas.py:93-101: the batches sampled in epoch 1 are
                                        #  kept in HBM and put back in later epochs -- graph_step.BatchCache)
                                        cache_batches=total_epoch > 1, num_neighbors=num_neighbors, sample_seed=self.seed)
            optimizer, wavg = graph_step.opt, graph_step.wavg
        elif controls:
            from .optim import FusedAdam, WeightAverage
            optimizer = FusedAdam(self.model.parameters(), lr=lr, weight_decay=weight_decay,                 # (the captured step's kernels)
                                  **{k: v for k, v in controls.items() if k != 'weight_average'})
            if weight_average is not None:
                wavg = WeightAverage(self.model, optimizer, weight_average)
        else:
            optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, weight_decay=weight_decay)   # kgwas.py:116
        ld_w = self._ld_weight_vector()
        min_val = -1000
        self.best_model = deepcopy(self.model).to(self.device)
        self.avg_model = wavg.avg_model if wavg is not None else None
        batches = graph_step.n_batches if graph_step is not None else len(self.train_loader)
        dropout = getattr(self.model, 'gat_dropout', 0.0) > 0 or getattr(self.model, 'gnn_dropout', 0.0) > 0
        print_sys('Start Training...')
        for ep in range(total_epoch):
            self.model.train()
            if num_neighbors is not None or epoch_order != 'fixed':  # (a finite fan-out draws anew every epoch, a shuffle orders anew)
                (graph_step if graph_step is not None else self.train_loader).set_epoch(ep)
            elif dropout and graph_step is not None:                 # (so do the dropout masks, on the same batches)
                graph_step.set_epoch(ep)
            steps = range(graph_step.n_batches) if graph_step is not None else enumerate(self.train_loader)
            for item in steps:
                if graph_step is not None:
                    step, loss = item, graph_step.step(item)
                    if step % 128 == 127:                    # a batch that outgrew the static layout: stop soon, not at the end
                        graph_step.poll()                    # of the epoch (no stream sync: the answer is read one poll later)
                else:
                    step, batch = item
                    if dropout:                              # (the word the captured step copies in: the same masks either way)
                        self.model.set_dropout_word(dropout_word(self.seed, ep, step))
                    loss = self.train_step(batch, optimizer, ld_w, world, loss_rule)
                    if wavg is not None:
                        wavg.update()                        # (behind the launch that advanced the counter, as in the captured step)
                if self.wandb:
                    self.wandb.log({'training_loss': loss.item()})
                if (step % 500 == 0) and (step >= 500):
                    print_sys('Epoch {} Step {} Train Loss: {:.4f}'.format(ep + 1, step + 1, loss.item()))
            if graph_step is not None:
                graph_step.check()
            if controlled:                                           # (the stream is synchronised here anyway)
                self.last_lr = float(optimizer.last_lr)
                if self.wandb:
                    self.wandb.log({'lr': self.last_lr})
            # (the averaged weights from the first averaging event on: host arithmetic on the updates done, nothing is read back)
            shown = self.avg_model if wavg is not None and wavg.started((ep + 1) * batches) else self.model
            val_res = evaluate_minibatch_clean(self.val_loader, shown, self.device)
            val_metrics = self._metrics(val_res, self._observed_rows(self.val_loader, len(val_res['pred'])))
            print_sys('Epoch {}: Validation MSE: {:.4f} Validation Pearson: {:.4f}. '.format(
                ep + 1, val_metrics['mse'], val_metrics['pearsonr']))
            self.val_metrics = val_metrics
            if self.wandb:
                for i, j in val_metrics.items():
                    if i != 'per_trait':
                        self.wandb.log({'val_' + i: j})
            if val_metrics['pearsonr'] > min_val:                    # kgwas.py:170-173
                min_val = val_metrics['pearsonr']
                self.best_model = deepcopy(shown)
        if save_best_model and rank == 0:
            save_model_path = os.path.join(self.data_path, 'model')
            print_sys('Saving models to ' + os.path.join(save_model_path, save_name))
            save_model(self.best_model, self.config, os.path.join(save_model_path, save_name))
        test_res = evaluate_minibatch_clean(self.test_loader, self.best_model, self.device)
        self.test_metrics = self._metrics(test_res, self._observed_rows(self.test_loader, len(test_res['pred'])))
        if self.wandb:
            for i, j in self.test_metrics.items():
                if i != 'per_trait':
                    self.wandb.log({'test_' + i: j})
        infer_res = evaluate_minibatch_clean(self.infer_loader, self.best_model, self.device)
        if self.model.lin.out_features != 1 or getattr(self.data, 'trait_observed', None) is not None:
            return self._postprocess_traits(infer_res['pred'], save_name)
        self.data.lr_uni['pred'] = infer_res['pred']                 # kgwas.py:191
        self._postprocess(save_name, save_best_model and rank == 0)

    def _observed_rows(self, loader, n):
        """bool [n, T]: which traits observe the first ``n`` input nodes of ``loader`` (the rows of its evaluation), or None for a
        data object without per-trait SNP lists."""
        observed = getattr(self.data, 'trait_observed', None)
        if observed is None:
            return None
        by_snp = np.zeros((int(self.data.data['SNP'].x.shape[0]), observed.shape[1]), dtype=bool)
        by_snp[np.asarray(self.data.all_ids, dtype=np.int64)] = observed
        return by_snp[torch.as_tensor(loader.ids).cpu().numpy()[:n]]

    def _metrics(self, res, observed=None):
        """compute_metrics of one evaluation; with T > 1 label columns: the metrics of every column under 'per_trait' and their
        means under the usual keys -- the best model is the one with the highest MEAN validation Pearson over the traits.
        ``observed`` (bool [n, T], per-trait SNP lists): trait t's metrics run over the rows it observes; a trait with fewer than
        two of them gets nan and stays out of the means; no trait left is an error."""
        if observed is None:
            if self.model.lin.out_features == 1:
                return compute_metrics(res, False, -1, -1, F.mse_loss)
            per = [compute_metrics({'pred': res['pred'][:, t], 'truth': res['truth'][:, t]}, False, -1, -1, F.mse_loss)
                   for t in range(res['pred'].shape[1])]
            return {'mse': float(np.mean([m['mse'] for m in per])), 'pearsonr': float(np.mean([m['pearsonr'] for m in per])),
                    'per_trait': per}
        pred, truth = np.asarray(res['pred']), np.asarray(res['truth'])
        pred, truth = pred.reshape(len(pred), -1), truth.reshape(len(truth), -1)
        per = []
        for t in range(pred.shape[1]):
            o = np.asarray(observed[:, t], dtype=bool)
            if o.sum() < 2:
                per.append({'mse': float('nan'), 'pearsonr': float('nan')})
            else:
                per.append(compute_metrics({'pred': pred[o, t], 'truth': truth[o, t]}, False, -1, -1, F.mse_loss))
        live = [m for m in per if not np.isnan(m['mse'])]
        if not live:
            raise ValueError('no trait observes two or more labels in this split: no metric can be computed')
        return {'mse': float(np.mean([m['mse'] for m in live])), 'pearsonr': float(np.mean([m['pearsonr'] for m in live])),
                'per_trait': per}

    def _postprocess_traits(self, pred, save_name):
        """``_postprocess`` once per label column: trait t's summary statistics (KGWAS_Data.trait_table) with column t of the
        predictions, written to <save_name>_trait<t>_pred.csv; ``kgwas_res`` becomes the list of the T tables.  With per-trait SNP
        lists a table holds the rows its trait observes; ``trait_pred`` keeps the whole matrix [len(all_ids), T], the predictions
        for the unobserved pairs included."""
        base = self.data.lr_uni
        pred = np.asarray(pred).reshape(len(pred), -1)
        self.trait_pred = pred
        tables = []
        per_trait_rows = getattr(self.data, 'trait_observed', None) is not None
        for t in range(pred.shape[1]):
            if per_trait_rows:                      # (a trait's table is cut from the base table, not from the previous trait's)
                self.data.lr_uni = base
            self.data.lr_uni = self.data.trait_table(t)
            self.data.lr_uni['pred'] = pred[self.data.trait_rows(t), t]
            self._postprocess(f'{save_name}_trait{t}', False)
            tables.append(self.kgwas_res)
        self.data.lr_uni = base
        self.kgwas_res = tables

    def get_network_weight(self):
        """The graph-side half of kgwas/kgwas.py:268-273: per-edge raw attention weights of the best model."""
        return get_network_weight(self, self.data)

    def get_disease_critical_network(self, variant_threshold=5e-8, magma_path=None, magma_threshold=0.05,
                                     program_threshold=0.05, K_neighbors=3, num_cpus=1):
        """kgwas/kgwas.py:268-273: (attention table, variant interpretation, disease-critical network).  The attention pass
        runs on the fused kernels (get_network_weight), the tables are host work (utils.generate_viz); the MAGMA / GSEA filter
        (``magma_path``) is not built."""
        from .utils import generate_viz
        df_network_weight = get_network_weight(self, self.data)
        df_variant_interpretation, disease_critical_network = generate_viz(
            self, df_network_weight, self.data_path, variant_threshold, magma_path, magma_threshold, program_threshold,
            K_neighbors, num_cpus)
        return df_network_weight, df_variant_interpretation, disease_critical_network

    def _postprocess(self, save_name, save_best_model):
        """kgwas.py:192-212: prediction-weighted p-values (Storey-Tibshirani pi0 per prediction-quantile bin,
        500 bins), bisection calibration, clip to [0,1], CSVs."""
        import numpy as np
        from .eval_utils import find_closest_x, storey_ribshirani_integrate
        lr_uni_to_save = deepcopy(self.data.lr_uni)
        self.data.lr_uni['abs_pred'] = np.abs(self.data.lr_uni['pred'])
        self.data.lr_uni['SR_P_val'] = storey_ribshirani_integrate(self.data.lr_uni, column='abs_pred', num_bins=500)
        self.data.lr_uni['SR'] = -(np.log10(self.data.lr_uni['SR_P_val'].astype(float).values))
        lr_uni_to_save['P_weighted'] = self.data.lr_uni['SR_P_val']
        scale_factor = find_closest_x(lr_uni_to_save)
        lr_uni_to_save['KGWAS_P'] = (scale_factor * lr_uni_to_save['P_weighted']).clip(lower=0, upper=1)
        out_dir = os.path.join(self.data_path, 'model_pred', 'new_experiments')
        self.kgwas_res = lr_uni_to_save
        if kdist.rank_world()[0] != 0:          # multi-GPU: every rank holds the results, rank 0 alone writes the files
            return
        try:
            os.makedirs(out_dir, exist_ok=True)
            write_tsv(lr_uni_to_save, os.path.join(out_dir, save_name + '_pred.csv'))      # (= to_csv(index=False, sep='\t'), same bytes)
            print('KGWAS prediction and p-values saved to ' + os.path.join(out_dir, save_name + '_pred.csv'))
            if save_best_model:
                write_tsv(lr_uni_to_save, os.path.join(self.data_path, 'model', save_name, 'pred.csv'))
        except OSError as e:   # read-only data_path: keep results in memory
            print_sys(f'could not write predictions: {e}')
