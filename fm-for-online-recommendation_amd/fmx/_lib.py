"""ctypes binding of libfmx.so (include/fmx.h).  There is no fallback: a missing library is an ImportError."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FMX_LIB_PATH") or os.path.join(_HERE, "libfmx.so")  # FMX_LIB_PATH: another build of the same ABI (A/B timing)

# enums of include/fmx.h
OK, ERR_ARG, ERR_SHAPE, ERR_ALIGN, ERR_LAUNCH, ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5
LAYOUT_WEIGHTS, LAYOUT_FTRL, LAYOUT_MOMENTS = 0, 1, 2
RULE_SIGNADAM, RULE_SGD, RULE_FTRL, RULE_ADAGRAD, RULE_ADAM = 0, 1, 2, 3, 4
LOSS_NONE, LOSS_BCE_LOGITS, LOSS_BCE_SIGMOID = 0, 1, 2

RULES = {"signadam": RULE_SIGNADAM, "sgd": RULE_SGD, "ftrl": RULE_FTRL, "adagrad": RULE_ADAGRAD, "adam": RULE_ADAM}
ADAPTIVE_RULES = ("adagrad", "adam")      # persistent per-coordinate state: tables in the moments layout
LAYOUTS = {"weights": LAYOUT_WEIGHTS, "ftrl": LAYOUT_FTRL, "moments": LAYOUT_MOMENTS}
LOSSES = {None: LOSS_NONE, "none": LOSS_NONE, "logits": LOSS_BCE_LOGITS, "sigmoid": LOSS_BCE_SIGMOID}
LIST_MAX_G = 16      # rows per list of fmx_fm_list_*: one positive and up to 15 negatives

EXPORTS = ["fmx_version", "fmx_last_error_string", "fmx_set_option", "fmx_sorted_width", "fmx_sorted_bbits", "fmx_workspace_bytes",
           "fmx_fm_forward", "fmx_mlp_forward", "fmx_mlp_fit", "fmx_mlp_hedge_fit", "fmx_mlp_section",
           "fmx_mlp_section_workspace_bytes", "fmx_fm_online_run", "fmx_online_run_mlp", "fmx_mlp_forward_batch", "fmx_mlp_hedge_section",
           "fmx_sort_occurrences", "fmx_fm_update", "fmx_fm_step", "fmx_fm_stream", "fmx_deepfm_stream", "fmx_stream_read",
           "fmx_fm_forward_partial", "fmx_fm_forward_finish", "fmx_sftrl_run", "fmx_sftrl_grid",
           "fmx_ftrl_dense_run", "fmx_ftrl_dense_grid", "fmx_rrf_run", "fmx_rrf_grid",
           "fmx_gather_read", "fmx_comm_unique_id", "fmx_comm_create", "fmx_comm_destroy", "fmx_owner_prefetch", "fmx_owner_step",
           "fmx_fm_topk_workspace_bytes", "fmx_fm_topk", "fmx_mlp_topk_workspace_bytes", "fmx_mlp_topk",
           "fmx_fm_update_occ", "fmx_afm_forward", "fmx_afm_workspace_bytes", "fmx_afm_step",
           "fmx_afm_side", "fmx_afm_topk_workspace_bytes", "fmx_afm_topk", "fmx_mlp_section_opt", "fmx_deepfm_stream_opt",
           "fmx_mlp_fit_opt", "fmx_online_run_mlp_opt", "fmx_afm_step_opt", "fmx_afm_stream", "fmx_afm_online_run",
           "fmx_fm_rank_workspace_bytes", "fmx_fm_rank", "fmx_mlp_rank_workspace_bytes", "fmx_mlp_rank",
           "fmx_afm_rank_workspace_bytes", "fmx_afm_rank",
           "fmx_fm_pair_forward", "fmx_fm_pair_step", "fmx_fm_pair_stream", "fmx_fm_pair_online_run",
           "fmx_mlp_pair_section", "fmx_deepfm_pair_stream", "fmx_mlp_pair_fit", "fmx_online_run_mlp_pair",
           "fmx_afm_pair_forward", "fmx_afm_pair_step", "fmx_afm_pair_step_opt", "fmx_afm_pair_stream", "fmx_afm_pair_online_run",
           "fmx_afm_pair_online_form", "fmx_fm_mine_negatives",
           "fmx_fm_list_workspace_bytes", "fmx_fm_list_forward", "fmx_fm_list_step", "fmx_fm_list_stream",
           "fmx_fm_list_online_run", "fmx_update_order",
           "fmx_fm_list_forward_q", "fmx_fm_list_step_q", "fmx_fm_list_stream_q", "fmx_alias_sample_negatives",
           "fmx_afm_list_workspace_bytes", "fmx_afm_list_forward", "fmx_afm_list_step", "fmx_afm_list_step_opt",
           "fmx_afm_list_stream", "fmx_afm_list_online_run",
           "fmx_fm_inbatch_splits", "fmx_fm_inbatch_lse_bytes", "fmx_fm_inbatch_forward", "fmx_fm_inbatch_backward",
           "fmx_fm_inbatch_occ_grad", "fmx_fm_inbatch_workspace_bytes", "fmx_fm_inbatch_step", "fmx_fm_inbatch_stream",
           "fmx_fm_inbatch_bank_splits", "fmx_fm_inbatch_bank_lse_bytes", "fmx_fm_inbatch_bank_forward", "fmx_fm_inbatch_bank_backward",
           "fmx_fm_inbatch_bank_push", "fmx_fm_inbatch_bank_workspace_bytes", "fmx_fm_inbatch_bank_step", "fmx_fm_inbatch_bank_stream",
           "fmx_mlp_list_section", "fmx_deepfm_list_stream", "fmx_mlp_list_fit", "fmx_online_run_mlp_list"]
ITEM_BANK_MAX = 1 << 20      # FMX_ITEM_BANK_MAX: the largest capacity of an item bank


I64_RETURNS = ("fmx_workspace_bytes", "fmx_mlp_section_workspace_bytes", "fmx_fm_topk_workspace_bytes",
               "fmx_mlp_topk_workspace_bytes", "fmx_afm_workspace_bytes", "fmx_afm_topk_workspace_bytes",
               "fmx_fm_rank_workspace_bytes", "fmx_mlp_rank_workspace_bytes", "fmx_afm_rank_workspace_bytes",
               "fmx_fm_list_workspace_bytes", "fmx_afm_list_workspace_bytes",
               "fmx_fm_inbatch_lse_bytes", "fmx_fm_inbatch_workspace_bytes",
               "fmx_fm_inbatch_bank_lse_bytes", "fmx_fm_inbatch_bank_workspace_bytes")   # byte counts: int64_t in include/fmx.h


class FmxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfmx error {code}: {msg}")
        self.code = code


class Table(C.Structure):
    _fields_ = [("rows", C.c_void_p), ("field_offsets", C.c_void_p), ("bias", C.c_void_p), ("n_rows", C.c_int64),
                ("n_fields", C.c_int32), ("k", C.c_int32), ("kp", C.c_int32), ("row_stride", C.c_int32),
                ("layout", C.c_int32), ("z_offset", C.c_int32), ("max_field_rows", C.c_int64),
                ("sort_offsets", C.c_void_p), ("sort_cols", C.c_void_p), ("n_sort_fields", C.c_int32), ("reserved", C.c_int32),
                ("max_sort_field_rows", C.c_int64), ("field_cols", C.c_void_p), ("field_base", C.c_void_p),
                ("n_cols", C.c_int32), ("reserved2", C.c_int32)]


class Hyper(C.Structure):
    _fields_ = [("lr", C.c_float), ("eps", C.c_float), ("alpha", C.c_float), ("beta", C.c_float),
                ("l1", C.c_float), ("l2", C.c_float),
                ("beta1", C.c_float), ("beta2", C.c_float), ("step", C.c_int32), ("reserved", C.c_int32)]   # (appended: read for the adam rule only)


class Mlp(C.Structure):
    _fields_ = [("params", C.c_void_p), ("n_layers", C.c_int32), ("k", C.c_int32), ("hidden", C.c_int32),
                ("reserved", C.c_int32)]


class MlpOpt(C.Structure):
    _fields_ = [("m", C.c_void_p), ("v", C.c_void_p), ("lr", C.c_float), ("eps", C.c_float), ("beta1", C.c_float),
                ("beta2", C.c_float), ("rule", C.c_int32), ("step", C.c_int32)]


class FwdOut(C.Structure):
    _fields_ = ([(n, C.c_void_p) for n in ("S", "bi", "first", "sfirst", "sbi", "logit", "loss", "dz", "error")]
                + [("sample_ld", C.c_int32), ("reserved", C.c_int32)])


class ItemBank(C.Structure):
    _fields_ = [("S", C.c_void_p), ("a", C.c_void_p), ("corr", C.c_void_p), ("key", C.c_void_p), ("state", C.c_void_p),
                ("capacity", C.c_int32), ("kp", C.c_int32)]


class Afm(C.Structure):
    _fields_ = [("params", C.c_void_p), ("k", C.c_int32), ("t", C.c_int32)]


class OwnerBufs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("parts_send", "parts_recv", "rec_local", "rec_all")]


COMM_ID_BYTES, COMM_SLOTS = 128, 4

_lib = None


def load():
    """Load libfmx.so once.  Raises ImportError when it has not been built (python __graft_entry__.py)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: build it with `make -C fm-for-online-recommendation_amd/csrc` "
                          "(or __graft_entry__.build()); fmx has no CPU or PyTorch fallback")
    lib = C.CDLL(LIB_PATH)
    p, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    TP, HP, FP = C.POINTER(Table), C.POINTER(Hyper), C.POINTER(FwdOut)
    lib.fmx_version.restype = C.c_int
    lib.fmx_last_error_string.restype = C.c_char_p
    lib.fmx_set_option.argtypes = [C.c_char_p, C.c_int]
    lib.fmx_sorted_width.argtypes = [C.c_int]
    lib.fmx_sorted_bbits.argtypes = [C.c_int]
    lib.fmx_update_order.argtypes = [p, i32, i32, p]
    lib.fmx_workspace_bytes.argtypes = [TP, i32]
    lib.fmx_fm_forward.argtypes = [TP, HP, p, p, p, i32, i32, f32, FP, p]
    lib.fmx_sort_occurrences.argtypes = [TP, p, i32, p, i64, p, p]
    lib.fmx_sftrl_run.argtypes = [p, p, i32, i32, i32, i32, C.c_double, C.c_double, i32, p, p, p, p, p, p, p, p]
    lib.fmx_sftrl_grid.argtypes = [p, p, i32, i32, i32, i32, p, p, i32, C.c_double, i32, p, p, p, p, p, p, p, p]
    lib.fmx_ftrl_dense_run.argtypes = [p, p, i32, i32, i32, C.c_double, i32, p, p, p, p, p, p, p]
    lib.fmx_ftrl_dense_grid.argtypes = [p, p, i32, i32, i32, p, p, i32, i32, p, p, p, p, p, p, p]
    lib.fmx_rrf_run.argtypes = [p, p, i32, i32, i32, C.c_double, C.c_double, i32, p, p, p, p, p, p]
    lib.fmx_rrf_grid.argtypes = [p, p, i32, i32, i32, p, p, p, i32, i32, p, p, p, p, p, p]
    lib.fmx_fm_forward_partial.argtypes = [TP, p, p, i32, i32, i32, i32, p, p, p]
    lib.fmx_fm_forward_finish.argtypes = [HP, p, i32, i32, p, i64, i32, p, i32, i32, f32, FP, p]
    lib.fmx_fm_update.argtypes = [TP, HP, i32, p, i64, p, p, p, p, p, i32, i32, p, f32, p, p]
    lib.fmx_fm_step.argtypes = [TP, HP, i32, i32, p, p, p, i32, f32, p, i64, FP, p, p]
    lib.fmx_fm_stream.argtypes = [TP, HP, i32, i32, p, p, i32, i32, f32, i32, p, i64, FP, p, C.POINTER(C.c_float), p]
    lib.fmx_stream_read.argtypes = [p, i64, p, p]
    lib.fmx_gather_read.argtypes = [p, i64, i32, i64, C.c_uint32, p, p]
    lib.fmx_fm_online_run.argtypes = [TP, HP, i32, i32, p, p, p, i32, p, p, p, p]
    lib.fmx_comm_unique_id.argtypes = [p]
    lib.fmx_comm_create.argtypes = [p, i32, i32, p, i32, C.POINTER(C.c_void_p)]
    lib.fmx_comm_destroy.argtypes = [p]
    lib.fmx_owner_prefetch.argtypes = [p, TP, p, i32, i32, p, p, i64, p, p]
    lib.fmx_owner_step.argtypes = [p, TP, HP, i32, i32, p, p, i32, i32, p, i64, C.POINTER(OwnerBufs), p, p, p]
    MP = C.POINTER(Mlp)
    lib.fmx_online_run_mlp.argtypes = [TP, HP, i32, i32, MP, i32, i32, f32, f32, p, p, p, p, i32, p, i64, FP, p, p, p]
    lib.fmx_mlp_forward.argtypes = [MP, p, i32, p, i32, p, p, p]
    lib.fmx_mlp_fit.argtypes = [MP, HP, i32, i32, p, i32, p, p, i32, f32, p, p, p, p]
    lib.fmx_mlp_hedge_fit.argtypes = [MP, f32, f32, f32, p, p, i32, p, p, i32, p, p]
    lib.fmx_mlp_forward_batch.argtypes = [MP, p, i32, p, i32, p, p, p, p]
    lib.fmx_mlp_hedge_section.argtypes = [MP, f32, f32, f32, p, p, i32, p, p, i32, p, p, p, p]
    lib.fmx_mlp_section_workspace_bytes.restype = C.c_int64
    lib.fmx_mlp_section_workspace_bytes.argtypes = [MP, i32]
    lib.fmx_mlp_section.argtypes = [MP, i32, p, i32, p, p, i32, f32, p, p, p, p, i32, p, f32, p, p]
    lib.fmx_deepfm_stream.argtypes = [TP, HP, i32, MP, i32, i32, p, p, i32, i32, f32, i32, p, i64, p, FP, p, p, p, f32, p, p]
    OP = C.POINTER(MlpOpt)
    lib.fmx_mlp_section_opt.argtypes = [MP, i32, p, i32, p, p, i32, f32, p, i64, p, p, p, i32, p, OP, p, p]
    lib.fmx_deepfm_stream_opt.argtypes = [TP, HP, i32, MP, i32, i32, p, p, i32, i32, f32, i32, p, i64, p, i64, FP, p, p, p, OP, p, p]
    lib.fmx_mlp_fit_opt.argtypes = [MP, HP, i32, p, i32, p, p, i32, f32, p, p, p, OP, p]
    lib.fmx_online_run_mlp_opt.argtypes = [TP, HP, i32, i32, MP, i32, p, p, p, i32, p, i64, FP, p, p, OP, p]
    lib.fmx_fm_topk_workspace_bytes.argtypes = [i32, i32, i32]
    lib.fmx_fm_topk.argtypes = [p, i32, p, i32, p, i32, p, i32, i32, p, p, i32, p, i64, p, p, p]
    lib.fmx_mlp_topk_workspace_bytes.argtypes = [MP, i32, i32, i32]
    lib.fmx_mlp_topk.argtypes = [MP, i32, p, p, i32, p, i32, p, p, i32, p, i32, i32, p, p, i32, p, i64, p, p, p]
    AP = C.POINTER(Afm)
    lib.fmx_fm_update_occ.argtypes = [TP, HP, i32, p, i64, p, p, p, i32, i32, p, f32, p, p]
    lib.fmx_afm_forward.argtypes = [TP, AP, HP, p, p, p, i32, i32, f32, p, p, p, p]
    lib.fmx_afm_workspace_bytes.argtypes = [TP, AP, i32]
    lib.fmx_afm_step.argtypes = [TP, HP, i32, AP, p, p, p, i32, f32, p, i64, p, p, p, p]
    lib.fmx_afm_step_opt.argtypes = [TP, HP, i32, AP, p, p, p, i32, f32, p, i64, p, OP, p, p, p]
    lib.fmx_afm_stream.argtypes = [TP, HP, i32, AP, p, p, p, i32, i32, f32, i32, p, i64, p, OP, p, p, p]
    lib.fmx_afm_online_run.argtypes = [TP, HP, i32, AP, p, p, p, i32, p, i64, p, OP, p, p, p, p]
    lib.fmx_afm_side.argtypes = [TP, AP, HP, p, p, i32, p, i32, i32, p, p, p, p]
    lib.fmx_afm_topk_workspace_bytes.argtypes = [AP, i32, i32, i32, i32, i32]
    lib.fmx_afm_topk.argtypes = [AP, p, p, i32, i32, p, p, i32, i32, i32, p, p, i32, p, i64, p, p, p]
    lib.fmx_fm_rank_workspace_bytes.argtypes = [i32, i32, i32]
    lib.fmx_fm_rank.argtypes = [p, i32, p, i32, p, i32, p, i32, i32, p, p, p, i32, i32, p, i64, p, p, p, p]
    lib.fmx_mlp_rank_workspace_bytes.argtypes = [MP, i32, i32, i32]
    lib.fmx_mlp_rank.argtypes = [MP, i32, p, p, i32, p, i32, p, p, i32, p, i32, i32, p, p, p, i32, i32, p, i64, p, p, p, p]
    lib.fmx_afm_rank_workspace_bytes.argtypes = [AP, i32, i32, i32, i32, i32]
    lib.fmx_afm_rank.argtypes = [AP, p, p, i32, i32, p, p, i32, i32, i32, p, p, p, i32, i32, p, i64, p, p, p, p]
    lib.fmx_fm_pair_forward.argtypes = [TP, HP, p, p, i32, f32, f32, FP, p]
    lib.fmx_fm_pair_step.argtypes = [TP, HP, i32, p, p, i32, f32, f32, p, i64, FP, p, p]
    lib.fmx_fm_pair_stream.argtypes = [TP, HP, i32, p, i32, i32, f32, f32, i32, p, i64, FP, p, p]
    lib.fmx_fm_pair_online_run.argtypes = [TP, HP, i32, p, p, i32, f32, p, p, p, p, p]
    lib.fmx_mlp_pair_section.argtypes = [MP, p, i32, p, i32, f32, f32, p, i64, p, p, p, i32, p, f32, OP, p, p]
    lib.fmx_deepfm_pair_stream.argtypes = [TP, HP, i32, MP, i32, p, i32, i32, f32, f32, i32, p, i64, p, i64, FP, p, p, p, f32, OP, p, p]
    lib.fmx_mlp_list_section.argtypes = [MP, p, i32, p, p, i32, i32, f32, p, i64, p, p, p, i32, p, f32, OP, p, p]
    lib.fmx_deepfm_list_stream.argtypes = [TP, HP, i32, MP, i32, p, i32, i32, i32, p, f32, i32, p, i64, p, i64, FP, p, p, p, f32, OP, p, p]
    lib.fmx_mlp_pair_fit.argtypes = [MP, HP, i32, p, i32, p, i32, f32, f32, p, p, p, p, OP, p]
    lib.fmx_online_run_mlp_pair.argtypes = [TP, HP, i32, MP, i32, p, p, i32, f32, p, i64, FP, p, p, p, p, OP, p]
    lib.fmx_mlp_list_fit.argtypes = [MP, HP, i32, p, i32, p, p, i32, i32, f32, p, p, p, p, p, OP, p]
    lib.fmx_online_run_mlp_list.argtypes = [TP, HP, i32, MP, i32, p, p, p, i32, i32, p, i64, FP, p, p, p, p, OP, p]
    lib.fmx_afm_pair_forward.argtypes = [TP, AP, HP, p, p, i32, f32, f32, p, p, p, p, p]
    lib.fmx_afm_pair_step.argtypes = [TP, HP, i32, AP, p, p, i32, f32, f32, p, i64, p, p, p, p, p]
    lib.fmx_afm_pair_step_opt.argtypes = [TP, HP, i32, AP, p, p, i32, f32, f32, p, i64, p, OP, p, p, p, p]
    lib.fmx_afm_pair_stream.argtypes = [TP, HP, i32, AP, p, p, i32, i32, f32, f32, i32, p, i64, p, OP, p, p, p]
    lib.fmx_afm_pair_online_run.argtypes = [TP, HP, i32, AP, p, p, i32, f32, p, i64, p, OP, p, p, p, p]
    lib.fmx_afm_pair_online_form.argtypes = [TP, AP, i32, C.POINTER(C.c_int32)]
    lib.fmx_fm_mine_negatives.argtypes = [p, i32, p, i32, p, i32, p, i32, i32, p, p, p, i32, i32, C.c_uint64, C.c_uint64, C.c_uint32,
                                          p, p, p]
    lib.fmx_fm_list_workspace_bytes.argtypes = [TP, i32, i32]
    lib.fmx_fm_list_forward.argtypes = [TP, HP, p, p, i32, i32, f32, FP, p]
    lib.fmx_fm_list_step.argtypes = [TP, HP, i32, p, p, i32, i32, f32, p, i64, FP, p, p]
    lib.fmx_fm_list_stream.argtypes = [TP, HP, i32, p, i32, i32, i32, f32, i32, p, i64, FP, p, p]
    lib.fmx_fm_list_online_run.argtypes = [TP, HP, i32, p, p, i32, i32, p, p, p, p, p]
    lib.fmx_fm_list_forward_q.argtypes = [TP, HP, p, p, p, i32, i32, f32, FP, p]
    lib.fmx_fm_list_step_q.argtypes = [TP, HP, i32, p, p, p, i32, i32, f32, p, i64, FP, p, p]
    lib.fmx_fm_list_stream_q.argtypes = [TP, HP, i32, p, p, i32, i32, i32, f32, i32, p, i64, FP, p, p]
    lib.fmx_alias_sample_negatives.argtypes = [p, p, p, i32, p, p, p, i32, i32, i32, C.c_uint64, C.c_uint64, C.c_uint32, p, p, p]
    lib.fmx_afm_list_workspace_bytes.argtypes = [TP, AP, i32, i32]
    lib.fmx_afm_list_forward.argtypes = [TP, AP, HP, p, p, i32, i32, f32, p, p, p, p, p]
    lib.fmx_afm_list_step.argtypes = [TP, HP, i32, AP, p, p, i32, i32, f32, p, i64, p, p, p, p, p]
    lib.fmx_afm_list_step_opt.argtypes = [TP, HP, i32, AP, p, p, i32, i32, f32, p, i64, p, OP, p, p, p, p]
    lib.fmx_afm_list_stream.argtypes = [TP, HP, i32, AP, p, p, i32, i32, i32, f32, i32, p, i64, p, OP, p, p, p]
    lib.fmx_afm_list_online_run.argtypes = [TP, HP, i32, AP, p, p, i32, i32, p, i64, p, OP, p, p, p, p]
    lib.fmx_fm_inbatch_splits.argtypes = [i32, i32]
    lib.fmx_fm_inbatch_lse_bytes.argtypes = [i32, i32]
    lib.fmx_fm_inbatch_forward.argtypes = [p, i32, p, p, i32, p, i32, i32, p, p, f32, p, i64, p, p, p]
    lib.fmx_fm_inbatch_backward.argtypes = [p, i32, p, p, i32, p, i32, i32, p, p, f32, p, i64, p, p, p, p]
    lib.fmx_fm_inbatch_occ_grad.argtypes = [TP, p, p, p, i32, p, p, p, p, i32, i32, p, i32, p]
    lib.fmx_fm_inbatch_workspace_bytes.argtypes = [TP, i32, i32]
    lib.fmx_fm_inbatch_step.argtypes = [TP, HP, i32, p, p, p, i32, p, p, i32, f32, p, i64, FP, p, p]
    lib.fmx_fm_inbatch_stream.argtypes = [TP, HP, i32, p, p, i32, p, p, i32, i32, f32, i32, p, i64, FP, p, p]
    BP = C.POINTER(ItemBank)
    lib.fmx_fm_inbatch_bank_splits.argtypes = [i32, i32]
    lib.fmx_fm_inbatch_bank_lse_bytes.argtypes = [i32, i32, i32]
    lib.fmx_fm_inbatch_bank_forward.argtypes = [p, i32, p, p, i32, p, i32, i32, p, p, BP, f32, p, i64, p, p, p, p]
    lib.fmx_fm_inbatch_bank_backward.argtypes = [p, i32, p, p, i32, p, i32, i32, p, p, BP, f32, p, i64, p, p, p, p]
    lib.fmx_fm_inbatch_bank_push.argtypes = [BP, p, i32, p, p, p, p, i32, p]
    lib.fmx_fm_inbatch_bank_workspace_bytes.argtypes = [TP, i32, i32, i32]
    lib.fmx_fm_inbatch_bank_step.argtypes = [TP, HP, i32, p, p, p, i32, p, p, BP, i32, f32, p, i64, FP, p, p]
    lib.fmx_fm_inbatch_bank_stream.argtypes = [TP, HP, i32, p, p, i32, p, p, BP, i32, i32, f32, i32, p, i64, FP, p, p]
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name in I64_RETURNS:
            fn.restype = C.c_int64
        elif name != "fmx_last_error_string":
            fn.restype = C.c_int
    _lib = lib
    return lib


def check(rc):
    if rc != OK:
        raise FmxError(rc, load().fmx_last_error_string().decode())
    return rc
