"""ctypes binding of libkgwas_hip.so (include/kgwas_hip.h).  Fails loudly when the library is missing:
there is NO CPU fallback for the product path."""
from __future__ import annotations

import ctypes as C
import os

KGW_MAX_TYPES = 8
KGW_MAX_RELS = 64
KGW_MAX_LAYERS = 4
KGW_CHUNK = 128
KGW_TILE = 1024
KGW_C = 128
KGW_MT_MAX = 32          # label columns of the multi-trait read-out (kgw_readout_wmse_mt_*)
PART_STRIDE = 132

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('KGW_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libkgwas_hip.so')     # (override: A/B runs of two builds)


class KgwGraph(C.Structure):
    _fields_ = [
        ('n_types', C.c_int32), ('n_rels', C.c_int32), ('n_layers', C.c_int32), ('n_hops', C.c_int32),
        ('n_nodes', C.c_int32 * KGW_MAX_TYPES),
        ('node_base', C.c_int32 * (KGW_MAX_TYPES + 1)),
        ('R_dst', C.c_int32 * KGW_MAX_TYPES),
        ('R_src', C.c_int32 * KGW_MAX_TYPES),
        ('rel_src', C.c_int32 * KGW_MAX_RELS),
        ('rel_dst', C.c_int32 * KGW_MAX_RELS),
        ('rel_slot_dst', C.c_int32 * KGW_MAX_RELS),
        ('rel_slot_src', C.c_int32 * KGW_MAX_RELS),
        ('rowptr_off', C.c_int64 * KGW_MAX_RELS),
        ('col_off', C.c_int64 * KGW_MAX_RELS),
        ('rel_live', (C.c_uint8 * KGW_MAX_RELS) * KGW_MAX_LAYERS),
        ('static_layout', C.c_int32),
        ('cap_rows', (C.c_int32 * KGW_MAX_TYPES) * KGW_MAX_LAYERS),
        ('cap_src', (C.c_int32 * KGW_MAX_TYPES) * KGW_MAX_LAYERS),
        ('short_types', C.c_uint32),
        ('g_rowptr', C.c_void_p),
        ('g_col', C.c_void_p),
    ]


class KgwBatchMeta(C.Structure):
    _fields_ = [
        ('hop_cnt', (C.c_int32 * (KGW_MAX_LAYERS + 1)) * KGW_MAX_TYPES),
        ('node_off', (C.c_int32 * (KGW_MAX_LAYERS + 2)) * KGW_MAX_TYPES),
        ('seg_off', (C.c_int32 * (KGW_MAX_RELS + 1)) * KGW_MAX_LAYERS),
        ('seg_end', C.c_int32 * KGW_MAX_LAYERS),
        ('edge_end', C.c_int32 * KGW_MAX_LAYERS),
        ('chunk_end', C.c_int32 * KGW_MAX_LAYERS),
        ('multi_cnt', C.c_int32 * KGW_MAX_LAYERS),
        ('n_rows', (C.c_int32 * KGW_MAX_TYPES) * KGW_MAX_LAYERS),
        ('z_base', (C.c_int32 * (KGW_MAX_TYPES + 1)) * KGW_MAX_LAYERS),
        ('n_src', (C.c_int32 * KGW_MAX_TYPES) * KGW_MAX_LAYERS),
        ('src_base', (C.c_int32 * (KGW_MAX_TYPES + 1)) * KGW_MAX_LAYERS),
        ('t_base', (C.c_int32 * (KGW_MAX_TYPES + 1)) * KGW_MAX_LAYERS),
        ('lay_rows', (C.c_int32 * KGW_MAX_TYPES) * KGW_MAX_LAYERS),
        ('lay_src', (C.c_int32 * KGW_MAX_TYPES) * KGW_MAX_LAYERS),
        ('n_chunks', C.c_int32 * KGW_MAX_LAYERS),
        ('n_edges', C.c_int32 * KGW_MAX_LAYERS),
        ('t_entries', C.c_int32 * KGW_MAX_LAYERS),
        ('cur', C.c_int32 * 8),
        ('error', C.c_int32),
        ('pad_', C.c_int32 * 3),
    ]


class KgwChunk(C.Structure):
    _fields_ = [('e0', C.c_int32), ('e1', C.c_int32), ('row', C.c_int32), ('rel', C.c_int32),
                ('first', C.c_int32), ('nch', C.c_int32), ('gpos_lo', C.c_int32), ('gpos_hi', C.c_int32)]


class KgwBatchBuf(C.Structure):
    _fields_ = [
        ('g2l', C.c_void_p), ('n_id', C.c_void_p), ('seg_deg', C.c_void_p), ('seg_nch', C.c_void_p),
        ('seg_ptr', C.c_void_p), ('seg_chptr', C.c_void_p), ('col_local', C.c_void_p),
        ('chunks', C.c_void_p), ('multi', C.c_void_p),
        ('t_cnt', C.c_void_p * KGW_MAX_LAYERS), ('t_ptr', C.c_void_p * KGW_MAX_LAYERS),
        ('t_edge', C.c_void_p * KGW_MAX_LAYERS), ('t_zrow', C.c_void_p * KGW_MAX_LAYERS),
        ('t_rel', C.c_void_p * KGW_MAX_LAYERS),
        ('scan_tmp', C.c_void_p), ('t_tmp', C.c_void_p), ('meta', C.c_void_p), ('meta_host', C.c_void_p),
        ('seg_cap', C.c_int64), ('edge_cap', C.c_int64), ('chunk_cap', C.c_int64),
        ('multi_cap', C.c_int64), ('trow_cap', C.c_int64), ('scan_cap', C.c_int64),
        ('grid_blocks', C.c_int32), ('pad_', C.c_int32),
    ]


class KgwLayerArgs(C.Structure):
    _fields_ = [
        ('layer', C.c_int32), ('n_chunks', C.c_int32), ('n_multi_hops', C.c_int32), ('n_src_rows', C.c_int32),
        ('neg_slope', C.c_float), ('inv_temp', C.c_float), ('flags', C.c_int32), ('n_heads', C.c_int32),
        ('graph_host', C.c_void_p), ('meta_host', C.c_void_p), ('meta_dev', C.c_void_p),
        ('chunks', C.c_void_p), ('multi', C.c_void_p), ('multi_cap', C.c_int64),
        ('col_local', C.c_void_p), ('H', C.c_void_p), ('a_dst', C.c_void_p), ('V', C.c_void_p), ('U', C.c_void_p),
        ('Z', C.c_void_p), ('stat', C.c_void_p), ('e_edge', C.c_void_p), ('part', C.c_void_p),
        ('dZ', C.c_void_p), ('adp', C.c_void_p), ('da_dst', C.c_void_p), ('part_da', C.c_void_p),
        ('t_ptr', C.c_void_p), ('t_edge', C.c_void_p), ('t_zrow', C.c_void_p),
        ('dH', C.c_void_p), ('ev_before', C.c_void_p), ('ev_after', C.c_void_p), ('da_src', C.c_void_p),
        ('logit_bias', C.c_void_p), ('partial_rels', C.c_uint64),
        ('t_rel', C.c_void_p), ('oct_flags', C.c_void_p), ('rel_sums', C.c_void_p),
        ('part_du', C.c_void_p), ('seg_chptr', C.c_void_p), ('duv_ws', C.c_void_p), ('dU', C.c_void_p), ('dV', C.c_void_p),
        ('drop_word_dev', C.c_void_p), ('drop_thresh', C.c_uint32), ('drop_scale', C.c_float),
    ]


class KgwEdgeAttr(C.Structure):
    _fields_ = [('attr', C.c_void_p), ('attr_off', C.c_int64 * KGW_MAX_RELS), ('dim', C.c_int32), ('pad_', C.c_int32),
                ('w', C.c_void_p), ('term', C.c_void_p), ('d_term', C.c_void_p), ('d_term_stride', C.c_int64),
                ('d_w', C.c_void_p), ('workspace', C.c_void_p)]


class KgwTnJob(C.Structure):
    _fields_ = [('A', C.c_void_p), ('lda', C.c_int64), ('B', C.c_void_p), ('ldb', C.c_int64), ('rows', C.c_int64),
                ('C', C.c_void_p), ('ldc', C.c_int64), ('colsum_a', C.c_void_p), ('colsum_ld', C.c_int64),
                ('workspace', C.c_void_p), ('workspace_floats', C.c_int64), ('rows_dev', C.c_void_p),
                ('M', C.c_int32), ('N', C.c_int32), ('c_transposed', C.c_int32), ('colsum_repeat', C.c_int32)]


class KgwGradSrc(C.Structure):
    _fields_ = [('ws', C.c_void_p), ('kind', C.c_int32), ('nblk', C.c_int32), ('M', C.c_int32), ('N', C.c_int32), ('MT', C.c_int32),
                ('NT', C.c_int32), ('gy', C.c_int32), ('gz', C.c_int32), ('K1', C.c_int32), ('c_transposed', C.c_int32),
                ('packed', C.c_void_p), ('flip', C.c_int32), ('pad_', C.c_int32)]


KGW_SEGCOPY_MAX = 40


class KgwSegCopy(C.Structure):
    _fields_ = [('n', C.c_int32), ('to_slot', C.c_int32), ('ptr', C.c_void_p * KGW_SEGCOPY_MAX), ('units', C.c_int64 * KGW_SEGCOPY_MAX),
                ('slot_off', C.c_int64 * KGW_SEGCOPY_MAX), ('slots', C.c_void_p), ('slot_stride', C.c_int64), ('slot_index', C.c_void_p)]


ADAM_FUSED_MAX, ADAM_FUSED_SRC, ADAM_FUSED_COUNTERS = 40, 12, 65 * 32     # include/kgwas_hip.h: KGW_ADAM_FUSED_*

KGW_LR_CONSTANT, KGW_LR_LINEAR, KGW_LR_COSINE, KGW_LR_STEP = 0, 1, 2, 3    # KgwLrSchedule.kind
LR_KINDS = {'constant': KGW_LR_CONSTANT, 'linear': KGW_LR_LINEAR, 'cosine': KGW_LR_COSINE, 'step': KGW_LR_STEP}
GRAD_NORM_UNIT = 1024                                                     # KGW_GRAD_NORM_UNIT


class KgwLrSchedule(C.Structure):
    _fields_ = [('kind', C.c_int32), ('warmup_steps', C.c_int32), ('total_steps', C.c_int32), ('step_size', C.c_int32),
                ('min_ratio', C.c_float), ('gamma', C.c_float)]


class KgwOptimCtl(C.Structure):
    _fields_ = [('sched', KgwLrSchedule), ('grad_scale_dev', C.c_void_p), ('lr_out_dev', C.c_void_p)]


KGW_AVG_EMA, KGW_AVG_SWA = 0, 1                                           # KgwWeightAvg.kind (include/kgwas_hip.h)
AVG_KINDS = {'ema': KGW_AVG_EMA, 'swa': KGW_AVG_SWA}
WEIGHT_AVG_MAX, WEIGHT_AVG_UNIT = 64, 1024                                # KGW_WEIGHT_AVG_MAX, KGW_WEIGHT_AVG_UNIT


class KgwWeightAvg(C.Structure):
    _fields_ = [('kind', C.c_int32), ('start_step', C.c_int32), ('every', C.c_int32), ('warmup', C.c_int32), ('decay', C.c_float)]


class KgwReadoutFold(C.Structure):
    _fields_ = [('scratch', C.c_void_p), ('terms', C.c_void_p), ('dw_lin', C.c_void_p), ('db_lin', C.c_void_p), ('loss', C.c_void_p),
                ('nb', C.c_int32), ('n', C.c_int32)]


KGW_LOSS_MSE, KGW_LOSS_HUBER = 0, 1                                       # KgwReadoutLossArgs.loss_kind (include/kgwas_hip.h)
LOSS_KINDS = {'mse': KGW_LOSS_MSE, 'huber': KGW_LOSS_HUBER}
READOUT_LOSS_ARGS_BYTES = 288                                             # KGW_READOUT_LOSS_ARGS_BYTES


class KgwReadoutLossArgs(C.Structure):
    _fields_ = [('H', C.c_void_p), ('W', C.c_void_p), ('b', C.c_void_p), ('n_id', C.c_void_p), ('y', C.c_void_p), ('w', C.c_void_p),
                ('pred_in', C.c_void_p), ('grad_loss', C.c_void_p), ('pred', C.c_void_p), ('loss', C.c_void_p), ('dH', C.c_void_p),
                ('dW', C.c_void_p), ('db', C.c_void_p), ('terms', C.c_void_p), ('scratch', C.c_void_p),
                ('fold_out', C.POINTER(KgwReadoutFold)), ('rows', C.c_int64), ('n', C.c_int32), ('T', C.c_int32), ('relu', C.c_int32),
                ('w_cols', C.c_int32), ('loss_kind', C.c_int32), ('reserved', C.c_int32), ('delta', C.c_float * 32)]


class KgwTnReducePlan(C.Structure):
    _fields_ = [('valid', C.c_int32), ('blocks', C.c_int32), ('reserved', C.c_int32 * 2), ('opaque', C.c_int64 * 96)]


class KgwSplitKJob(C.Structure):
    _fields_ = [('X', C.c_void_p), ('ldx', C.c_int64), ('W', C.c_void_p), ('ldw', C.c_int64), ('bias', C.c_void_p),
                ('Y', C.c_void_p), ('ldy', C.c_int64), ('rows', C.c_int64), ('seg_stat', C.c_void_p), ('gamma', C.c_void_p),
                ('dgamma', C.c_void_p), ('K', C.c_int32), ('N', C.c_int32), ('relu', C.c_int32), ('w_is_kn', C.c_int32)]


class KgwRelvecJob(C.Structure):
    _fields_ = [('n_rels_total', C.c_int32), ('n_live', C.c_int32), ('n_blk', C.c_int32), ('duv_pieces', C.c_int32),
                ('live_of_rel', C.c_void_p), ('rel_ids', C.c_void_p), ('bip_pos', C.c_void_p),
                ('w_src_t', C.c_void_p), ('w_dst_t', C.c_void_p), ('att_src', C.c_void_p), ('att_dst', C.c_void_p),
                ('U_full', C.c_void_p), ('V', C.c_void_p), ('bias', C.c_void_p), ('blk_of_live', C.c_void_p), ('bias_sum', C.c_void_p),
                ('zero_buf', C.c_void_p), ('zero_floats', C.c_int64),
                ('dU_full', C.c_void_p), ('dV', C.c_void_p), ('dw_src_acc', C.c_void_p),
                ('dw_src_t', C.c_void_p), ('dw_dst_t', C.c_void_p), ('datt_src', C.c_void_p), ('datt_dst', C.c_void_p)]


class KgwHDropJob(C.Structure):
    _fields_ = [('src', C.c_void_p), ('lds', C.c_int64), ('dst', C.c_void_p), ('ldd', C.c_int64), ('rows', C.c_int32), ('type', C.c_int32)]


class KgwLNormJob(C.Structure):
    _fields_ = [('src', C.c_void_p), ('lds', C.c_int64), ('dst', C.c_void_p), ('ldd', C.c_int64), ('rows', C.c_int32), ('type', C.c_int32),
                ('weight', C.c_void_p), ('bias', C.c_void_p), ('stat', C.c_void_p)]


class KgwLNormBwdJob(C.Structure):
    _fields_ = [('g', C.c_void_p), ('ldg', C.c_int64), ('y', C.c_void_p), ('ldy', C.c_int64), ('out', C.c_void_p), ('ldo', C.c_int64),
                ('dy', C.c_void_p), ('lddy', C.c_int64), ('rows', C.c_int32), ('type', C.c_int32), ('weight', C.c_void_p),
                ('stat', C.c_void_p)]


class KgwRootJob(C.Structure):
    _fields_ = [('x', C.c_void_p), ('ldx', C.c_int64), ('y', C.c_void_p), ('ldy', C.c_int64), ('dst', C.c_void_p), ('ldd', C.c_int64),
                ('rows', C.c_int32), ('type', C.c_int32), ('W', C.c_void_p)]


class KgwRootBwdJob(C.Structure):
    _fields_ = [('g', C.c_void_p), ('ldg', C.c_int64), ('out', C.c_void_p), ('ldo', C.c_int64), ('x', C.c_void_p), ('ldx', C.c_int64),
                ('gm', C.c_void_p), ('ldgm', C.c_int64), ('dx', C.c_void_p), ('lddx', C.c_int64), ('rows', C.c_int32),
                ('type', C.c_int32), ('W', C.c_void_p), ('x_premasked', C.c_int32), ('reserved', C.c_int32)]


class KgwFoldArgs(C.Structure):
    _fields_ = [('n', C.c_int32), ('n_rels', C.c_int32), ('n_mlp', C.c_int32), ('duv_pieces', C.c_int32),
                ('rel_ids_host', C.c_void_p), ('src_mlp_host', C.c_void_p), ('dst_mlp_host', C.c_void_p),
                ('w_src_t', C.c_void_p), ('fc_weight', C.c_void_p * 4), ('fc_bias', C.c_void_p * 4),
                ('U', C.c_void_p), ('V', C.c_void_p),
                ('Up', C.c_void_p), ('Vp', C.c_void_p), ('kappa', C.c_void_p), ('Wp', C.c_void_p), ('gamma', C.c_void_p),
                ('dUp', C.c_void_p), ('dVp', C.c_void_p), ('dkappa', C.c_void_p), ('dWp', C.c_void_p), ('dgamma', C.c_void_p),
                ('dU', C.c_void_p), ('dV', C.c_void_p), ('dws', C.c_void_p),
                ('d_fc_weight', C.c_void_p * 4), ('d_fc_bias', C.c_void_p * 4)]


EXPORTS = ['kgw_version', 'kgw_status_string', 'kgw_struct_sizes', 'kgw_sample_batch', 'kgw_sample_batch_parts', 'kgw_sample_batch_fanout', 'kgw_epoch_order', 'kgw_sampler_scan_ints', 'kgw_segments_copy',
           'kgw_softmax_pack', 'kgw_softmax_merge', 'kgw_scatter_rows', 'kgw_linear_splitk', 'kgw_linear_splitk_workspace_floats', 'kgw_linear_splitk_ind', 'kgw_ind_colsum', 'kgw_linear_splitk_multi', 'kgw_ind_colsum_multi', 'kgw_fold_fwd', 'kgw_fold_bwd', 'kgw_relation_sums',
           'kgw_gat_aggregate_fwd', 'kgw_gat_aggregate_bwd_dst', 'kgw_gat_aggregate_bwd_src',
           'kgw_edge_term_fwd', 'kgw_edge_term_bwd', 'kgw_edge_term_workspace_floats', 'kgw_gat_aggregate_fwd_eterm',
           'kgw_gather_rows', 'kgw_gather_rows_multi', 'kgw_scatter_relu_rows', 'kgw_scatter_relu_rows_workspace_floats', 'kgw_edge_alpha', 'kgw_debug_reduce', 'kgw_debug_reduce8', 'kgw_tn_gemm', 'kgw_tn_gemm_ex', 'kgw_tn_gemm_multi', 'kgw_tn_gemm_workspace_floats', 'kgw_tn_gemm_partial', 'kgw_tn_gemm_multi_partial', 'kgw_tn_split', 'kgw_tn_direct_rows', 'kgw_param_tail', 'kgw_tn_reduce_launch', 'kgw_tn_gemm_partial_ride', 'kgw_transform_bwd_ex', 'kgw_mlp2_bwd_first_partial', 'kgw_mlp2_bwd_first_packed', 'kgw_adam_fused', 'kgw_gemm3_partial', 'kgw_gemm3_flip', 'kgw_transform_bwd', 'kgw_grad_finish',
           'kgw_linear', 'kgw_mlp2_fwd', 'kgw_mlp2w_fwd', 'kgw_mlp2_bwd_first', 'kgw_mlp2_bwd_first_workspace_floats', 'kgw_gemm3', 'kgw_gemm3_riders', 'kgw_gemm3_rider_blocks', 'kgw_gemm3_pack', 'kgw_gemm3_packed_bytes', 'kgw_gemm3_workspace_floats', 'kgw_adam', 'kgw_adam_notick', 'kgw_relvec_fwd', 'kgw_relvec_bwd', 'kgw_relvec_bwd_acc', 'kgw_relvec_fwd_multi', 'kgw_relvec_bwd_multi', 'kgw_wmse_fwd', 'kgw_wmse_bwd', 'kgw_readout_wmse_fwd', 'kgw_readout_wmse_bwd', 'kgw_readout_wmse_train', 'kgw_readout_wmse_train_parts', 'kgw_readout_train_fold', 'kgw_readout_mt_pred', 'kgw_readout_mt_pred_bwd', 'kgw_readout_wmse_mt_fwd', 'kgw_readout_wmse_mt_bwd',
           'kgw_readout_wmse_mt_train', 'kgw_readout_wmse_mtw_fwd', 'kgw_readout_wmse_mtw_bwd', 'kgw_readout_wmse_mtw_train',
           'kgw_accumulate_stats', 'kgw_accumulate_stats_tick', 'kgw_hidden_dropout',
           'kgw_layer_norm_relu_fwd', 'kgw_layer_norm_partial_floats', 'kgw_layer_norm_bwd', 'kgw_layer_norm_fold',
           'kgw_root_linear_fwd', 'kgw_root_linear_bwd',
           'kgw_adam_ctl', 'kgw_adam_fused_ctl', 'kgw_lr_at', 'kgw_grad_norm_partial', 'kgw_grad_norm_fold',
           'kgw_grad_norm_workspace_doubles', 'kgw_weight_avg_update', 'kgw_weight_avg_alpha',
           'kgw_readout_loss_fwd', 'kgw_readout_loss_bwd', 'kgw_readout_loss_train']

_lib = None


class KgwasHipError(RuntimeError):
    pass


def lib():
    """Load libkgwas_hip.so once.  Raises (never falls back) when it is absent or stale."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KgwasHipError(
            f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  kgwas_amd has no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    L.kgw_version.restype = C.c_int
    L.kgw_status_string.restype = C.c_char_p
    L.kgw_status_string.argtypes = [C.c_int]
    L.kgw_struct_sizes.argtypes = [C.POINTER(C.c_int64), C.c_int]
    sizes = (C.c_int64 * 7)()
    L.kgw_struct_sizes(sizes, 7)
    mine = [C.sizeof(KgwGraph), C.sizeof(KgwBatchMeta), C.sizeof(KgwChunk), C.sizeof(KgwBatchBuf),
            C.sizeof(KgwLayerArgs), C.sizeof(KgwTnJob), C.sizeof(KgwGradSrc)]
    # (an older library named by KGW_LIB_PATH for an A/B run ends KgwLayerArgs before the attention-dropout fields: it never reads
    #  them, so the longer mirror is safe to pass; ops.gat_aggregate refuses dropout= with such a library)
    L.kgw_has_dropout = True
    if 'KGW_LIB_PATH' in os.environ and sizes[4] == KgwLayerArgs.drop_word_dev.offset:
        L.kgw_has_dropout = False
        mine[4] = sizes[4]
    if list(sizes) != mine:
        raise KgwasHipError(f'ABI struct size mismatch: library {list(sizes)} vs binding {mine}')
    L.kgw_sample_batch.argtypes = [C.POINTER(KgwGraph), C.POINTER(KgwBatchBuf), C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_int32, C.c_void_p]
    L.kgw_sample_batch_parts.argtypes = [C.POINTER(KgwGraph), C.POINTER(KgwBatchBuf), C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    if hasattr(L, 'kgw_sample_batch_fanout'):       # (absent from an older library named by KGW_LIB_PATH for an A/B run)
        L.kgw_sample_batch_fanout.argtypes = [C.POINTER(KgwGraph), C.POINTER(KgwBatchBuf), C.c_void_p, C.c_int32, C.c_int32,
                                              C.POINTER(C.c_int32), C.c_void_p, C.c_void_p]
    if hasattr(L, 'kgw_epoch_order'):               # (absent from an older library named by KGW_LIB_PATH for an A/B run)
        L.kgw_epoch_order.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p,
                                      C.c_void_p]
    L.kgw_sampler_scan_ints.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    L.kgw_sampler_scan_ints.restype = C.c_int64
    L.kgw_segments_copy.argtypes = [C.POINTER(KgwSegCopy), C.c_int32, C.c_void_p]
    L.kgw_softmax_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.kgw_softmax_merge.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kgw_scatter_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    for name in ('kgw_gat_aggregate_fwd', 'kgw_gat_aggregate_bwd_dst', 'kgw_gat_aggregate_bwd_src'):
        getattr(L, name).argtypes = [C.POINTER(KgwLayerArgs), C.c_void_p]
    L.kgw_gather_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.kgw_tn_gemm_multi.argtypes = [C.c_int32, C.POINTER(KgwTnJob), C.c_void_p]
    L.kgw_scatter_relu_rows_workspace_floats.restype = C.c_int64
    L.kgw_scatter_relu_rows_workspace_floats.argtypes = [C.c_int64]
    L.kgw_scatter_relu_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kgw_gather_rows_multi.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int64), C.c_int32,
                                        C.POINTER(C.c_void_p), C.c_void_p]
    L.kgw_edge_alpha.argtypes = [C.POINTER(KgwLayerArgs), C.c_void_p, C.c_void_p]
    if hasattr(L, 'kgw_edge_term_fwd'):             # (absent from an older library named by KGW_LIB_PATH for an A/B run)
        L.kgw_edge_term_fwd.argtypes = [C.POINTER(KgwLayerArgs), C.POINTER(KgwEdgeAttr), C.c_void_p]
        L.kgw_edge_term_bwd.argtypes = [C.POINTER(KgwLayerArgs), C.POINTER(KgwEdgeAttr), C.c_void_p]
        L.kgw_edge_term_workspace_floats.argtypes = [C.POINTER(KgwLayerArgs)]
        L.kgw_edge_term_workspace_floats.restype = C.c_int64
        L.kgw_gat_aggregate_fwd_eterm.argtypes = [C.POINTER(KgwLayerArgs), C.c_void_p, C.c_void_p]
        s8 = (C.c_int64 * 8)()
        L.kgw_struct_sizes(s8, 8)
        if s8[7] != C.sizeof(KgwEdgeAttr):
            raise KgwasHipError(f'ABI struct size mismatch: KgwEdgeAttr library {s8[7]} vs binding {C.sizeof(KgwEdgeAttr)}')
    L.kgw_debug_reduce.argtypes = [C.c_void_p] * 5
    L.kgw_debug_reduce8.argtypes = [C.c_void_p] * 3
    L.kgw_tn_gemm_workspace_floats.restype = C.c_int64
    L.kgw_tn_gemm_workspace_floats.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.kgw_linear.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64,
                             C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                             C.c_void_p]
    L.kgw_mlp2_fwd.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                               C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                               C.c_void_p]
    L.kgw_mlp2w_fwd.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.kgw_gemm3_packed_bytes.restype = C.c_int64
    L.kgw_gemm3_packed_bytes.argtypes = [C.c_int64]
    L.kgw_gemm3_workspace_floats.restype = C.c_int64
    L.kgw_gemm3_workspace_floats.argtypes = [C.c_int64, C.c_int64]
    L.kgw_gemm3_pack.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.kgw_gemm3.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32,
                            C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.kgw_gemm3_riders.argtypes = L.kgw_gemm3.argtypes[:-1] + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    L.kgw_gemm3_rider_blocks.argtypes = [C.c_int64, C.c_int64]
    L.kgw_mlp2_bwd_first_workspace_floats.restype = C.c_int64
    L.kgw_mlp2_bwd_first_workspace_floats.argtypes = [C.c_int64]
    L.kgw_mlp2_bwd_first.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p]
    L.kgw_linear_splitk_workspace_floats.restype = C.c_int64
    L.kgw_linear_splitk_workspace_floats.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    L.kgw_linear_splitk.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                    C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.kgw_linear_splitk_ind.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                        C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.kgw_ind_colsum.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    L.kgw_linear_splitk_multi.argtypes = [C.c_int32, C.POINTER(KgwSplitKJob), C.c_void_p]
    L.kgw_ind_colsum_multi.argtypes = [C.c_int32, C.POINTER(KgwSplitKJob), C.c_void_p]
    L.kgw_relation_sums.argtypes = [C.POINTER(KgwLayerArgs), C.c_void_p, C.c_void_p, C.c_void_p]
    L.kgw_fold_fwd.argtypes = [C.POINTER(KgwFoldArgs), C.c_void_p]
    L.kgw_fold_bwd.argtypes = [C.POINTER(KgwFoldArgs), C.c_void_p]
    L.kgw_adam.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                           C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]
    L.kgw_adam_notick.argtypes = L.kgw_adam.argtypes
    L.kgw_relvec_fwd.argtypes = [C.c_int32] + [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.kgw_relvec_fwd_multi.argtypes = [C.c_int32, C.POINTER(KgwRelvecJob), C.c_void_p]
    L.kgw_relvec_bwd_multi.argtypes = [C.c_int32, C.POINTER(KgwRelvecJob), C.c_void_p]
    L.kgw_relvec_bwd.argtypes = [C.c_int32] + [C.c_void_p] * 12 + [C.c_int32, C.c_void_p]
    L.kgw_relvec_bwd_acc.argtypes = [C.c_int32] + [C.c_void_p] * 13 + [C.c_int32, C.c_void_p]
    L.kgw_tn_gemm.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                              C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    L.kgw_tn_gemm_ex.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                 C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p]
    L.kgw_tn_gemm_partial.argtypes = [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                      C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                      C.POINTER(KgwGradSrc), C.c_void_p]
    L.kgw_tn_gemm_multi_partial.argtypes = [C.c_int32, C.POINTER(KgwTnJob), C.POINTER(KgwGradSrc), C.c_void_p]
    L.kgw_param_tail.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    L.kgw_mlp2_bwd_first_partial.argtypes = L.kgw_mlp2_bwd_first.argtypes[:-1] + [C.POINTER(KgwGradSrc), C.c_void_p]
    L.kgw_mlp2_bwd_first_packed.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int32,
                                            C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                            C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    L.kgw_adam_fused.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(KgwGradSrc), C.c_void_p,
                                 C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    L.kgw_gemm3_partial.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                    C.POINTER(KgwGradSrc), C.c_void_p]
    L.kgw_gemm3_flip.restype = C.c_int
    L.kgw_grad_finish.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(KgwGradSrc), C.c_void_p]
    L.kgw_transform_bwd.argtypes = [C.c_int32, C.POINTER(KgwTnJob), C.c_int32, C.POINTER(KgwSplitKJob), C.c_int32, C.POINTER(KgwSplitKJob),
                                    C.c_void_p]
    L.kgw_transform_bwd_ex.argtypes = L.kgw_transform_bwd.argtypes[:-1] + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kgw_tn_reduce_launch.argtypes = [C.c_void_p, C.c_void_p]
    L.kgw_tn_direct_rows.restype = C.c_int64
    L.kgw_tn_direct_rows.argtypes = [C.c_int64]
    L.kgw_tn_gemm_partial_ride.argtypes = L.kgw_tn_gemm_partial.argtypes[:-1] + [C.c_void_p, C.c_void_p]
    L.kgw_wmse_fwd.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p]
    L.kgw_wmse_bwd.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kgw_readout_wmse_fwd.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4
    L.kgw_readout_wmse_bwd.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 6
    L.kgw_readout_wmse_train.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 8
    L.kgw_readout_wmse_train_parts.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int64, C.c_int32] + [C.c_void_p] * 9
    L.kgw_readout_train_fold.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, 'kgw_readout_wmse_mt_train'):     # (absent from an older library named by KGW_LIB_PATH for an A/B run)
        L.kgw_readout_mt_pred.argtypes = [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p] * 2
        L.kgw_readout_mt_pred_bwd.argtypes = [C.c_void_p] * 3 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 5
        L.kgw_readout_wmse_mt_fwd.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p] * 4
        L.kgw_readout_wmse_mt_bwd.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 6
        L.kgw_readout_wmse_mt_train.argtypes = [C.c_void_p] * 6 + [C.c_int32, C.c_int64, C.c_int32, C.c_int32] + [C.c_void_p] * 8
    if hasattr(L, 'kgw_readout_wmse_mtw_train'):    # (the same argument lists; w is [N_SNP][T])
        L.kgw_readout_wmse_mtw_fwd.argtypes = L.kgw_readout_wmse_mt_fwd.argtypes
        L.kgw_readout_wmse_mtw_bwd.argtypes = L.kgw_readout_wmse_mt_bwd.argtypes
        L.kgw_readout_wmse_mtw_train.argtypes = L.kgw_readout_wmse_mt_train.argtypes
    if hasattr(L, 'kgw_hidden_dropout'):            # (absent from an older library named by KGW_LIB_PATH for an A/B run)
        L.kgw_hidden_dropout.argtypes = [C.c_int32, C.POINTER(KgwHDropJob), C.c_int32, C.c_void_p, C.c_uint32, C.c_float, C.c_void_p]
    if hasattr(L, 'kgw_layer_norm_relu_fwd'):       # (absent likewise)
        L.kgw_layer_norm_relu_fwd.argtypes = [C.c_int32, C.POINTER(KgwLNormJob), C.c_int32, C.c_float, C.c_void_p]
        L.kgw_layer_norm_partial_floats.argtypes = [C.c_int32, C.POINTER(KgwLNormBwdJob)]
        L.kgw_layer_norm_partial_floats.restype = C.c_int64
        L.kgw_layer_norm_bwd.argtypes = [C.c_int32, C.POINTER(KgwLNormBwdJob), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
        L.kgw_layer_norm_fold.argtypes = [C.c_int32, C.POINTER(KgwLNormBwdJob), C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    if hasattr(L, 'kgw_root_linear_fwd'):           # (absent likewise)
        L.kgw_root_linear_fwd.argtypes = [C.c_int32, C.POINTER(KgwRootJob), C.c_int32, C.c_void_p]
        L.kgw_root_linear_bwd.argtypes = [C.c_int32, C.POINTER(KgwRootBwdJob), C.c_void_p]
    if hasattr(L, 'kgw_adam_ctl'):                  # (absent likewise)
        L.kgw_adam_ctl.argtypes = L.kgw_adam.argtypes[:-1] + [C.c_int32, C.POINTER(KgwOptimCtl), C.c_void_p]
        L.kgw_adam_fused_ctl.argtypes = L.kgw_adam_fused.argtypes[:-1] + [C.POINTER(KgwOptimCtl), C.c_void_p]
        L.kgw_lr_at.argtypes = [C.POINTER(KgwLrSchedule), C.c_float, C.c_int32]
        L.kgw_lr_at.restype = C.c_double
        L.kgw_grad_norm_workspace_doubles.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
        L.kgw_grad_norm_workspace_doubles.restype = C.c_int64
        L.kgw_grad_norm_partial.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p, C.c_int64, C.c_void_p]
        L.kgw_grad_norm_fold.argtypes = [C.c_void_p, C.c_int64, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        s10 = (C.c_int64 * 10)()
        L.kgw_struct_sizes(s10, 10)
        if [s10[8], s10[9]] != [C.sizeof(KgwLrSchedule), C.sizeof(KgwOptimCtl)]:
            raise KgwasHipError(f'ABI struct size mismatch: KgwLrSchedule / KgwOptimCtl library {[s10[8], s10[9]]} vs binding '
                                f'{[C.sizeof(KgwLrSchedule), C.sizeof(KgwOptimCtl)]}')
    if hasattr(L, 'kgw_weight_avg_update'):         # (absent likewise)
        L.kgw_weight_avg_update.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64), C.c_void_p,
                                            C.POINTER(KgwWeightAvg), C.c_void_p]
        L.kgw_weight_avg_alpha.argtypes = [C.POINTER(KgwWeightAvg), C.c_int32, C.POINTER(C.c_int32)]
        L.kgw_weight_avg_alpha.restype = C.c_float
        s11 = (C.c_int64 * 11)()
        L.kgw_struct_sizes(s11, 11)
        if s11[10] != C.sizeof(KgwWeightAvg):
            raise KgwasHipError(f'ABI struct size mismatch: KgwWeightAvg library {s11[10]} vs binding {C.sizeof(KgwWeightAvg)}')
    if hasattr(L, 'kgw_readout_loss_train'):        # (absent likewise)
        for name in ('kgw_readout_loss_fwd', 'kgw_readout_loss_bwd', 'kgw_readout_loss_train'):
            getattr(L, name).argtypes = [C.POINTER(KgwReadoutLossArgs), C.c_void_p]
        # (the library asserts the same constant where it is built: kgw_struct_sizes' list is closed at eleven entries)
        if C.sizeof(KgwReadoutLossArgs) != READOUT_LOSS_ARGS_BYTES:
            raise KgwasHipError(f'ABI struct size mismatch: KgwReadoutLossArgs header {READOUT_LOSS_ARGS_BYTES} vs binding '
                                f'{C.sizeof(KgwReadoutLossArgs)}')
    L.kgw_accumulate_stats.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.kgw_accumulate_stats_tick.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    _lib = L
    return L


KGW_E_UNSUPPORTED = -3
KGW_GRAD_G3T = 5                # KgwGradSrc.kind: partial sums of kgw_gemm3_partial (include/kgwas_hip.h)


def has_heads() -> bool:
    """Does the loaded library know KgwLayerArgs.n_heads?  (The field took the place of a padding word, so an older library named
    by KGW_LIB_PATH for an A/B run has the same struct size and would run one head.)  n_heads = 3 is refused by value before
    anything else is looked at; the older library sees an empty layer and returns 0.  No launch either way."""
    a = KgwLayerArgs()
    a.n_heads = 3
    return lib().kgw_gat_aggregate_fwd(C.byref(a), None) == -2


KGW_F_SIGMOID_GATE = 8          # KgwLayerArgs.flags (include/kgwas_hip.h)


def has_sigmoid_gate() -> bool:
    """Does the loaded library know KGW_F_SIGMOID_GATE?  The gate together with KGW_F_RAW_WEIGHTS is refused by value (-3) before
    anything else is looked at; a library that predates the flag (KGW_LIB_PATH of an A/B run) sees an empty raw-weights layer and
    returns 0.  No launch either way."""
    a = KgwLayerArgs()
    a.flags = KGW_F_SIGMOID_GATE | 1
    return lib().kgw_gat_aggregate_fwd(C.byref(a), None) == KGW_E_UNSUPPORTED


def has_edge_attr() -> bool:
    """Does the loaded library have the edge-attribute entry points (kgw_edge_term_fwd, kgw_edge_term_bwd,
    kgw_gat_aggregate_fwd_eterm)?  An older library named by KGW_LIB_PATH for an A/B run lacks the symbols."""
    return hasattr(lib(), 'kgw_gat_aggregate_fwd_eterm')


def has_hidden_dropout() -> bool:
    """Does the loaded library have kgw_hidden_dropout (hidden-state dropout between the layers)?  An older library named by
    KGW_LIB_PATH for an A/B run lacks the symbol."""
    return hasattr(lib(), 'kgw_hidden_dropout')


def has_layer_norm() -> bool:
    """Does the loaded library have the layer-normalisation kernels (kgw_layer_norm_relu_fwd / _bwd / _fold)?  An older library
    named by KGW_LIB_PATH for an A/B run lacks the symbols."""
    return hasattr(lib(), 'kgw_layer_norm_relu_fwd')


def has_root_weight() -> bool:
    """Does the loaded library have the root-weight kernels (kgw_root_linear_fwd / _bwd)?  An older library named by KGW_LIB_PATH
    for an A/B run lacks the symbols."""
    return hasattr(lib(), 'kgw_root_linear_fwd')


def has_optim_ctl() -> bool:
    """Does the loaded library have the optimiser controls (kgw_adam_ctl, kgw_adam_fused_ctl, kgw_grad_norm_partial / _fold:
    learning-rate schedules and gradient-norm clipping)?  An older library named by KGW_LIB_PATH for an A/B run lacks the symbols."""
    return hasattr(lib(), 'kgw_adam_ctl')


def has_weight_avg() -> bool:
    """Does the loaded library have kgw_weight_avg_update (the EMA / SWA shadow weights)?  An older library named by KGW_LIB_PATH
    for an A/B run lacks the symbol."""
    return hasattr(lib(), 'kgw_weight_avg_update')


def has_readout_loss() -> bool:
    """Does the loaded library have the read-out node with a loss kind (kgw_readout_loss_fwd / _bwd / _train: the Huber loss)?  An
    older library named by KGW_LIB_PATH for an A/B run lacks the symbols."""
    return hasattr(lib(), 'kgw_readout_loss_train')


KGW_ORDER_SEEDS, KGW_ORDER_BATCHES = 1, 2    # kgw_epoch_order's modes (include/kgwas_hip.h)
EPOCH_ORDER_BLOCK, EPOCH_ORDER_GRID = 256, 2048   # its launch: threads per block, most blocks (KGW_BLK, KGW_GRID of csrc/kgw_common.h)


def has_epoch_order() -> bool:
    """Does the loaded library have kgw_epoch_order (the per-epoch order of the training seeds)?  An older library named by
    KGW_LIB_PATH for an A/B run lacks the symbol."""
    return hasattr(lib(), 'kgw_epoch_order')


def check(status: int, what: str):
    if status != 0:
        msg = lib().kgw_status_string(int(status))
        raise KgwasHipError(f'{what} failed: status {status} ({msg.decode() if msg else "?"})')


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
