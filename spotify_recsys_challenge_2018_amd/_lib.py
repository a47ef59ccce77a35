"""ctypes binding of libdae_hip.so (C ABI: include/dae_hip.h).

There is NO CPU fallback: if the shared library is missing or a call fails, this raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdae_hip.so")

DAE_OUT_SCORE, DAE_OUT_LOGIT = 0, 1
# largest k (include/dae_hip.h): DAE_MAX_K for the exact mode, the title mix, the pipeline and the metrics kernel; DAE_MAX_K_DEEP for
# the fp32 / bf16 ranking calls, dae_topk_dense / dae_topk_merge and dae_rank_candidates
DAE_MAX_K, DAE_MAX_K_DEEP = 1024, 4096
DAE_DTYPE_F32, DAE_DTYPE_BF16, DAE_DTYPE_BF16_EXACT = 0, 1, 2
DAE_CAND_CHUNK = 256            # candidates of one row a workgroup of the candidate kernels takes (include/dae_hip.h)

# every symbol include/dae_hip.h declares (tests/test_abi_cpu.py checks the .so exports all of them)
EXPORTS = [
    "dae_version", "dae_create", "dae_destroy", "dae_set_stream", "dae_last_error",
    "dae_scratch_bytes", "dae_profile_enable", "dae_profile_read", "dae_profile_kernel", "dae_clock_probe", "dae_last_plan",
    "dae_coo_to_csr", "dae_seeds_from_csr", "dae_train_set_create", "dae_train_set_destroy", "dae_train_batch", "dae_train_set_attach_titles", "dae_train_titles", "dae_encode", "dae_prepack_decoder", "dae_prepack_decoder_rows", "dae_share_decoder", "dae_exact_bounds",
    "dae_exact_guard_read", "dae_exact_guard_words", "dae_exact_guard_snapshot", "dae_exact_stats_read", "dae_set_exact_margin", "dae_set_exact_margin_range", "dae_set_exact_audit", "dae_exact_audit_read",
    "dae_set_filter_skip", "dae_filter_skip_read", "dae_filter_skip_last", "dae_tile_bounds_read", "dae_sample_skip_read", "dae_live_proof_read", "dae_last_tau_read", "dae_decode_dense", "dae_decode_topk",
    "dae_score_topk", "dae_score_topk_begin", "dae_score_topk_finish", "dae_topk_dense", "dae_topk_merge", "dae_set_train_dtype", "dae_train_forward_backward",
    "dae_decode_loss_rows", "dae_score_loss", "dae_mix_loss_rows",
    "dae_train_shard_encode", "dae_train_shard_decode", "dae_train_shard_finish", "dae_title_features", "dae_title_prepack_features",
    "dae_mix_scores", "dae_decode_mix_term", "dae_set_score_mix", "dae_decode_mix_term_add", "dae_ensemble_topk", "dae_mix_topk_exact", "dae_mix_exact_shape_ok", "dae_title_score_exact", "dae_title_score", "dae_row_sums", "dae_mix_weights", "dae_title_loss_backward", "dae_title_loss_backward_cols", "dae_title_conv_backward", "dae_adam_step",
    "dae_adam_rows_begin", "dae_adam_rows_apply", "dae_adam_rows_flush", "dae_set_enc_grad_prezeroed",
    "dae_arm_decoder_adam", "dae_set_decode_gate", "dae_set_overlap_hint",
    "dae_pipeline_create", "dae_pipeline_create_titled", "dae_pipeline_destroy", "dae_pipeline_submit", "dae_pipeline_submit_titled", "dae_pipeline_flush", "dae_pipeline_poll",
    "dae_pipeline_release", "dae_pipeline_stats", "dae_pipeline_exact_margin", "dae_pipeline_times", "dae_pipeline_last_error",
    "dae_rank_metrics", "dae_pipeline_enable_eval", "dae_pipeline_submit_eval", "dae_pipeline_poll_eval",
    "dae_decode_candidates", "dae_score_candidates", "dae_mix_candidates", "dae_rank_candidates", "dae_candidates_unique",
    "dae_pipeline_enable_candidates", "dae_pipeline_submit_candidates", "dae_pipeline_poll_candidates",
    "dae_rank_of_plan", "dae_decode_rank_of", "dae_score_rank_of", "dae_mix_rank_of",
    "dae_ensemble_candidates", "dae_ensemble_rank_of",
    "dae_catalogue_create", "dae_catalogue_destroy", "dae_prepack_decoder_catalogue", "dae_score_topk_catalogue",
    "dae_decode_topk_catalogue", "dae_title_score_catalogue", "dae_pipeline_set_catalogue",
]
DAE_PIPE_BUSY = 1
DAE_PIPE_BAD_ID = 2             # dae_pipeline_poll_candidates: the feed's launch held an id outside -1 / [0, V) (its slot is a NaN)
DAE_CAND_UNIQUE_MAX_V = 1 << 20

_lib = None


class DaeError(RuntimeError):
    pass


def load():
    """Load libdae_hip.so; raise loudly if it has not been built (python -m <pkg>.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DaeError(
            "libdae_hip.so not found at %s -- build it with "
            "`python -m spotify_recsys_challenge_2018_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the scoring path." % LIB_PATH)
    # torch must come first: it brings its own libamdhip64; loading ours before it puts two HIP
    # runtimes in the process and the second one finds no device.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    c_int, c_i64, c_f, c_u32, vp = (ctypes.c_int, ctypes.c_int64, ctypes.c_float,
                                    ctypes.c_uint32, ctypes.c_void_p)
    lib.dae_version.restype = c_int
    lib.dae_create.argtypes = [c_int, ctypes.POINTER(vp)]
    lib.dae_destroy.argtypes = [vp]
    lib.dae_set_stream.argtypes = [vp, vp]
    lib.dae_last_error.argtypes = [vp]
    lib.dae_last_error.restype = ctypes.c_char_p
    lib.dae_scratch_bytes.argtypes = [vp]
    lib.dae_scratch_bytes.restype = ctypes.c_size_t
    lib.dae_profile_enable.argtypes = [vp, c_int]
    lib.dae_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int)]
    lib.dae_profile_kernel.argtypes = [vp]
    lib.dae_profile_kernel.restype = ctypes.c_char_p
    lib.dae_clock_probe.argtypes = [vp, vp, c_int, vp, ctypes.POINTER(c_int)]
    lib.dae_last_plan.argtypes = [ctypes.POINTER(ctypes.c_int32)]
    lib.dae_coo_to_csr.argtypes = [vp, vp, vp, c_int, c_i64, c_int, c_int, vp, vp, vp, vp]
    lib.dae_seeds_from_csr.argtypes = [vp, vp, vp, c_int, c_int, vp, vp]
    lib.dae_train_set_create.argtypes = [vp, vp, vp, vp, vp, c_int, c_int, c_int, ctypes.POINTER(vp)]
    lib.dae_train_set_destroy.argtypes = [vp]
    lib.dae_train_batch.argtypes = [vp, vp, vp, c_int, c_int, vp, vp, vp, c_int, vp, vp, vp, c_int, vp]
    lib.dae_train_set_attach_titles.argtypes = [vp, vp, c_int, c_int, c_int]
    lib.dae_train_titles.argtypes = [vp, vp, vp, c_int, vp]
    lib.dae_encode.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_f, c_f, c_u32, vp]
    lib.dae_prepack_decoder.argtypes = [vp, vp, vp, c_int, c_int, c_int, c_int, c_int]
    lib.dae_prepack_decoder_rows.argtypes = [vp, vp, vp, c_int, c_int, c_int, c_int]
    lib.dae_share_decoder.argtypes = [vp, vp, c_int]
    lib.dae_exact_bounds.argtypes = [vp, vp]
    lib.dae_exact_guard_read.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    lib.dae_exact_guard_words.argtypes = [vp, ctypes.POINTER(vp)]
    lib.dae_exact_guard_snapshot.argtypes = [vp, vp]
    lib.dae_set_exact_margin.argtypes = [vp, c_f]
    lib.dae_exact_stats_read.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.dae_set_exact_margin_range.argtypes = [vp, c_int, c_int, c_f]
    lib.dae_set_exact_audit.argtypes = [vp, c_int, c_int]
    lib.dae_exact_audit_read.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.dae_set_filter_skip.argtypes = [vp, c_int]
    lib.dae_filter_skip_read.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.dae_filter_skip_last.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), c_int, ctypes.POINTER(c_int)]
    lib.dae_sample_skip_read.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.dae_live_proof_read.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    lib.dae_last_tau_read.argtypes = [vp, ctypes.c_void_p, c_int]
    lib.dae_tile_bounds_read.argtypes = [vp, vp, c_int, ctypes.POINTER(c_int)]
    lib.dae_decode_dense.argtypes = [vp, vp, c_int, c_int, c_int, c_int, vp, c_i64]
    lib.dae_decode_topk.argtypes = [vp, vp, c_int, c_int, c_int, c_int, vp, vp, c_int, c_int, vp, vp]
    lib.dae_score_topk.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp, vp,
                                   c_int, c_int, vp, vp]
    lib.dae_score_topk_begin.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, vp, c_int, vp]
    lib.dae_score_topk_finish.argtypes = [vp, vp, vp, vp, c_int, vp, vp]
    lib.dae_topk_dense.argtypes = [vp, vp, c_i64, c_int, c_int, c_int, vp, vp, c_int, c_int, vp, vp]
    lib.dae_topk_merge.argtypes = [vp, c_int, c_int, c_int, vp, vp, c_int, vp, vp]
    lib.dae_set_train_dtype.argtypes = [vp, c_int]
    lib.dae_set_train_dtype.restype = c_int
    lib.dae_train_forward_backward.argtypes = (
        [vp] + [vp] * 6 + [vp] * 4 + [c_int] * 5 + [c_f, c_f, c_u32, c_f] + [vp] * 5)
    lib.dae_decode_loss_rows.argtypes = [vp, vp, c_int, c_int, c_int, vp, vp, vp, vp, vp, c_int, vp]
    lib.dae_score_loss.argtypes = (
        [vp] + [vp] * 6 + [vp] * 4 + [c_int] * 5 + [c_f, c_f, c_u32, c_f] + [vp] * 2)
    lib.dae_mix_loss_rows.argtypes = [vp, vp, vp, c_i64, c_int, vp, vp, vp, c_i64, vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, vp, vp, vp]
    lib.dae_train_shard_encode.argtypes = [vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_f, c_u32, vp]
    lib.dae_train_shard_decode.argtypes = (
        [vp, vp, vp] + [vp] * 3 + [vp] * 3 + [c_int] * 6 + [c_f, c_u32, c_f] + [vp] * 4)
    lib.dae_train_shard_finish.argtypes = (
        [vp, vp] + [vp] * 3 + [vp] * 4 + [c_int] * 5 + [c_f, c_f, c_u32, c_f] + [vp] * 4)
    lib.dae_title_features.argtypes = [vp, vp, c_int, c_int, vp, c_int, c_int, vp, vp, ctypes.POINTER(ctypes.c_int32),
                                       c_int, c_int, c_f, c_u32, vp, c_i64, vp, vp]
    lib.dae_title_prepack_features.argtypes = [vp, vp, c_int, c_int, vp, ctypes.POINTER(ctypes.c_int32), c_int, c_int]
    lib.dae_mix_scores.argtypes = [vp, vp, c_i64, vp, c_i64, vp, vp, c_int, c_int]
    lib.dae_decode_mix_term.argtypes = [vp, vp, c_int, c_int, c_int, vp, c_int, vp, c_i64]
    lib.dae_set_score_mix.argtypes = [vp, vp, c_i64, c_int, vp]
    lib.dae_decode_mix_term_add.argtypes = lib.dae_decode_mix_term.argtypes
    lib.dae_ensemble_topk.argtypes = [ctypes.POINTER(vp), c_int, ctypes.POINTER(vp), ctypes.POINTER(c_int), ctypes.POINTER(vp),
                                      vp, vp, c_int, vp, c_int, c_int, c_int, vp, vp, c_int, vp, vp]
    pvp, pci = ctypes.POINTER(vp), ctypes.POINTER(c_int)
    lib.dae_ensemble_candidates.argtypes = [pvp, c_int, pvp, pci, pvp, pvp, pvp, vp, vp, c_int, vp, vp, vp, c_int, c_int,
                                            vp, vp, c_int, vp, vp]
    lib.dae_ensemble_rank_of.argtypes = [pvp, c_int, pvp, pci, pvp, pvp, pvp, vp, vp, c_int, vp, vp, vp, c_int, c_int, c_int,
                                         vp, vp, c_int, vp, vp, c_int, vp, vp, vp]
    lib.dae_mix_topk_exact.argtypes = [vp, vp, vp, c_i64, vp, c_i64, c_int, vp, vp, c_int, vp, vp, c_int, vp, vp, vp]
    lib.dae_mix_exact_shape_ok.argtypes = [c_int, c_int]
    lib.dae_row_sums.argtypes = [vp, vp, vp, vp, c_int, c_f, c_u32, vp]
    lib.dae_title_score_exact.argtypes = [vp, vp, vp, vp, c_int, c_i64, c_int, c_int, vp, vp, c_int, vp, c_int, vp, c_int, c_int, vp, vp,
                                          ctypes.POINTER(ctypes.c_int32), c_int, c_int, c_int, vp, c_int, c_int, vp, vp, vp, vp]
    lib.dae_mix_weights.argtypes = [vp, vp, vp, vp, c_int, c_f, c_u32, vp, vp, vp]
    lib.dae_title_loss_backward.argtypes = [vp, vp, c_i64, vp, c_i64, vp, vp, vp, vp, vp, c_int, c_int, c_int,
                                            vp, c_int, vp, vp, vp, vp, vp]
    lib.dae_title_loss_backward_cols.argtypes = [vp, vp, c_i64, vp, c_i64, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int,
                                                 vp, c_int, vp, vp, vp, vp, vp]
    lib.dae_title_conv_backward.argtypes = [vp, vp, c_int, c_int, vp, c_int, c_int, vp, ctypes.POINTER(ctypes.c_int32),
                                            c_int, c_int, vp, vp, vp, c_i64, c_f, c_u32, vp, vp, vp]
    lib.dae_adam_step.argtypes = [vp, vp, vp, vp, vp, c_i64, c_f, c_f, c_f, c_f, c_int]
    lib.dae_adam_rows_begin.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, c_int, c_f, c_f, c_f, c_int]
    lib.dae_adam_rows_apply.argtypes = [vp, vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, c_int,
                                        c_f, c_f, c_f, c_f, c_int]
    lib.dae_adam_rows_flush.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_f, c_f, c_f, c_int]
    lib.dae_set_enc_grad_prezeroed.argtypes = [vp, c_int]
    lib.dae_arm_decoder_adam.argtypes = [vp, vp, vp, c_f, c_f, c_f, c_f, c_int]
    lib.dae_set_decode_gate.argtypes = [vp, vp, vp]
    lib.dae_set_overlap_hint.argtypes = [vp, c_int]
    u64p, i32pp, f32pp, ip = (ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)),
                              ctypes.POINTER(ctypes.POINTER(ctypes.c_float)), ctypes.POINTER(c_int))
    lib.dae_pipeline_create.argtypes = [c_int, vp, vp, vp, vp, c_int, c_int, c_int, c_int, c_int, c_int, c_i64, c_int, c_int, c_int,
                                        ctypes.POINTER(vp)]
    i32p = ctypes.POINTER(ctypes.c_int32)
    lib.dae_pipeline_create_titled.argtypes = ([c_int, vp, vp, vp, vp, c_int, c_int, c_int,        # device, the DAE's arrays, V, H, n_tracks
                                                vp, c_int, c_int, vp, vp, i32p, c_int, c_int,       # emb, n_char, E, conv_w, conv_b, filter_sizes, n_sizes, F
                                                vp, vp, c_int, c_int] +                             # Output_WT, Output_b, ld_feat, L
                                               [c_int] * 3 + [c_i64] + [c_int] * 3 + [ctypes.POINTER(vp)])
    lib.dae_pipeline_submit_titled.argtypes = [vp, vp, vp, c_int, c_i64, c_int, vp, vp, u64p]
    lib.dae_title_score.argtypes = [vp, vp, c_int, vp, vp, c_int, c_i64, c_int, c_int, vp, vp, c_int, vp, c_int, vp, c_int, c_int, vp, vp,
                                    i32p, c_int, c_int, c_int, vp, c_int, c_int, vp, vp, vp, vp]
    lib.dae_pipeline_destroy.argtypes = [vp]
    lib.dae_pipeline_submit.argtypes = [vp, vp, vp, c_int, c_i64, c_int, u64p]
    lib.dae_pipeline_flush.argtypes = [vp]
    lib.dae_pipeline_poll.argtypes = [vp, c_int, u64p, i32pp, f32pp, ip, ip]
    lib.dae_pipeline_release.argtypes = [vp, c_int]
    lib.dae_pipeline_stats.argtypes = [vp, u64p]
    lib.dae_pipeline_exact_margin.argtypes = [vp, c_f]
    lib.dae_pipeline_times.argtypes = [vp, u64p]
    lib.dae_pipeline_last_error.argtypes = [vp]
    lib.dae_rank_metrics.argtypes = [vp, vp, c_i64, c_int, c_int, vp, vp, vp, vp]
    lib.dae_pipeline_enable_eval.argtypes = [vp, vp, c_i64]
    lib.dae_pipeline_submit_eval.argtypes = [vp, vp, vp, c_int, c_i64, c_int, vp, vp, vp, vp, u64p]
    lib.dae_pipeline_poll_eval.argtypes = [vp, c_int, u64p, ctypes.POINTER(vp), ip, ip]
    lib.dae_pipeline_last_error.restype = ctypes.c_char_p
    lib.dae_decode_candidates.argtypes = [vp, vp, c_i64, c_int, c_int, vp, vp, c_int, vp, vp, c_int, c_int, vp, vp]
    lib.dae_score_candidates.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, vp, vp, c_int, c_int, vp, vp]
    lib.dae_mix_candidates.argtypes = [vp, vp, vp, c_i64, c_int, vp, vp, vp, c_i64, vp, vp, vp, vp, c_int, c_int, vp, vp,
                                       c_int, vp, vp]
    lib.dae_rank_candidates.argtypes = [vp, c_int, c_int, vp, vp, vp, c_int, vp, vp, c_int, c_int, vp, vp]
    lib.dae_candidates_unique.argtypes = [vp, c_int, c_int, vp, vp, vp, c_int]
    lib.dae_pipeline_enable_candidates.argtypes = [vp, c_i64, c_int, c_int]
    lib.dae_pipeline_submit_candidates.argtypes = [vp, vp, vp, c_int, c_i64, c_int, vp, vp, vp, vp, u64p]
    lib.dae_pipeline_poll_candidates.argtypes = [vp, c_int, u64p, f32pp, ctypes.POINTER(c_i64), ip, ip]
    lib.dae_rank_of_plan.argtypes = [c_int, c_int, c_int, ctypes.POINTER(ctypes.c_int32)]
    lib.dae_decode_rank_of.argtypes = [vp, vp, c_int, c_int, vp, vp, c_int, c_int, vp, vp, vp, vp, c_int, vp, vp, vp]
    lib.dae_score_rank_of.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, c_int, vp, vp, vp, vp, c_int, vp, vp, vp]
    lib.dae_mix_rank_of.argtypes = [vp, vp, vp, c_i64, c_int, vp, vp, vp, c_i64, vp, vp, vp, vp, c_int, c_int, c_int, vp, vp, vp, vp,
                                    c_int, vp, vp, vp]
    lib.dae_catalogue_create.argtypes = [vp, vp, c_int, c_int, ctypes.POINTER(vp)]
    lib.dae_catalogue_destroy.argtypes = [vp]
    lib.dae_prepack_decoder_catalogue.argtypes = [vp, vp, vp, vp, c_int, c_int, c_int]
    lib.dae_score_topk_catalogue.argtypes = [vp, vp, vp, vp, vp, vp, c_int, c_int, c_int, c_int, vp, vp, vp, c_int,
                                             c_int, c_int, vp, vp]
    lib.dae_decode_topk_catalogue.argtypes = [vp, vp, c_int, c_int, c_int, vp, vp, vp, c_int, c_int, c_int, vp, vp]
    lib.dae_title_score_catalogue.argtypes = lib.dae_title_score.argtypes + [vp]
    lib.dae_pipeline_set_catalogue.argtypes = [vp, vp]
    for name in EXPORTS:
        if name not in ("dae_last_error", "dae_scratch_bytes", "dae_profile_kernel", "dae_pipeline_last_error"):
            getattr(lib, name).restype = c_int
    _lib = lib
    return lib


def rank_of_plan(n_rows, hidden, n_ans):
    """How a rank_of call of these sizes is cut (dae_rank_of_plan; host only): {"rows": rows per row group of the counting
    launch, "capacity": answers of a row one pass of the GEMM takes, "row_groups", "blocks_per_group"}."""
    out = (ctypes.c_int32 * 4)()
    if load().dae_rank_of_plan(int(n_rows), int(hidden), int(n_ans), out):
        raise ValueError("rank_of_plan: no geometry for %d rows, hidden %d, %d answers" % (n_rows, hidden, n_ans))
    return {"rows": int(out[0]), "capacity": int(out[1]), "row_groups": int(out[2]), "blocks_per_group": int(out[3])}


def mix_exact_shape_ok(hidden, ld_feat):
    """Does the exact title mix (dae_mix_topk_exact) take a DAE of this hidden size with title feature rows of this length?
    The library's own rule (dae_mix_exact_shape_ok): no context, no device."""
    return bool(load().dae_mix_exact_shape_ok(int(hidden), int(ld_feat)))


def _ptr(t):
    """Device pointer of a torch tensor (or None)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


class TrainSet:
    """Owns one dae_train_set: the training playlists on the device of `ctx` (dae_train_set_create copies the host arrays
    once).  trk / art: the flat id arrays of the two sides, trk_off / art_off: n_playlists + 1 offsets each -- the reader's
    `_trk / _trk_off / _art / _art_off` (utils/data_reader.py).  Ids outside their ranges raise DaeError before any launch."""

    def __init__(self, ctx, trk, trk_off, art, art_off, n_tracks, n_items):
        import numpy as np
        self.ctx, self.h = ctx, None                         # (the context outlives the set: it names the device)
        trk, art = (np.ascontiguousarray(a, dtype=np.int64) for a in (trk, art))
        for a in (trk, art):                                 # narrowed for the device; what does not fit is no id
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise DaeError("dae_train_set_create: an id does not fit 32 bits")
        trk, art = trk.astype(np.int32), art.astype(np.int32)
        trk_off, art_off = (np.ascontiguousarray(a, dtype=np.int64) for a in (trk_off, art_off))
        if trk_off.size != art_off.size or trk_off.size < 2:
            raise DaeError("dae_train_set_create: trk_off and art_off hold n_playlists + 1 offsets each")
        if int(trk_off[-1]) != trk.size or int(art_off[-1]) != art.size:
            raise DaeError("dae_train_set_create: the last offset of a side is the length of its id array")
        self.n_playlists = int(trk_off.size) - 1
        h = ctypes.c_void_p()
        vp = ctypes.c_void_p
        ctx.check(ctx.lib.dae_train_set_create(ctx.h, vp(trk.ctypes.data), vp(trk_off.ctypes.data), vp(art.ctypes.data),
                                               vp(art_off.ctypes.data), self.n_playlists, int(n_tracks), int(n_items),
                                               ctypes.byref(h)))
        self.h = h
        self.has_titles, self.title_len = False, 0

    def attach_titles(self, titles, n_char):
        """The playlists' title rows join the set (dae_train_set_attach_titles copies them once): titles int
        [n_playlists, L], every entry -1 (no character) or a character id in [0, n_char).  Anything else, a second attach or
        rows for another number of playlists raise DaeError before any launch."""
        import numpy as np
        t = np.asarray(titles)
        if t.ndim != 2 or t.shape[0] != self.n_playlists:
            raise DaeError("dae_train_set_attach_titles: titles of shape %s for a set of %d playlists" % (t.shape, self.n_playlists))
        if t.size and (t.min() < -2 ** 31 or t.max() >= 2 ** 31):
            raise DaeError("dae_train_set_attach_titles: a character id does not fit 32 bits")
        t = np.ascontiguousarray(t, dtype=np.int32)
        rc = self.ctx.lib.dae_train_set_attach_titles(self.h, ctypes.c_void_p(t.ctypes.data), int(t.shape[0]), int(t.shape[1]),
                                                      int(n_char))
        if rc != 0:                                          # (a call without a context: its message is the global one)
            raise DaeError("libdae_hip error %d: %s" % (rc, self.ctx.lib.dae_last_error(None).decode()))
        self.has_titles, self.title_len = True, int(t.shape[1])

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dae_train_set_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns one dae_ctx bound to a device + the caller's current torch stream."""

    def __init__(self, device_index=0):
        import torch
        self.lib = load()
        if not torch.cuda.is_available():
            raise DaeError("no GPU visible: the DAE scoring path runs only on MI355X (gfx950)")
        h = ctypes.c_void_p()
        rc = self.lib.dae_create(int(device_index), ctypes.byref(h))
        if rc != 0:
            raise DaeError("dae_create failed (%d): %s"
                           % (rc, self.lib.dae_last_error(None).decode()))
        self.h = h
        self.device_index = int(device_index)
        self.bind_stream()

    def bind_stream(self):
        import torch
        s = torch.cuda.current_stream(self.device_index).cuda_stream
        self.check(self.lib.dae_set_stream(self.h, ctypes.c_void_p(s)))

    def check(self, rc):
        if rc != 0:
            raise DaeError("libdae_hip error %d: %s"
                           % (rc, self.lib.dae_last_error(self.h).decode()))

    def coo_to_csr(self, positions, values, n_rows, n_cols):
        """Device COO (feed order, duplicates: last wins) -> CSR.  positions: int64 [nnz,2] CUDA tensor,
        values: float32 [nnz] or [1].  Returns (row_ptr, col, val, status) CUDA tensors; col / val have
        room for nnz entries, row_ptr[n_rows] of them are valid.  status != 0: an index was out of range."""
        import torch
        nnz = int(positions.shape[0])
        dev = positions.device
        rp = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
        col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
        val = torch.empty(max(nnz, 1), dtype=torch.float32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        bcast = 1 if (values.numel() == 1 and nnz != 1) else 0
        self.check(self.lib.dae_coo_to_csr(self.h, _ptr(positions), _ptr(values), bcast, nnz, int(n_rows),
                                           int(n_cols), _ptr(rp), _ptr(col), _ptr(val), _ptr(status)))
        return rp, col, val, status

    def seeds_from_csr(self, row_ptr, col, n_tracks):
        """Seed CSR = the track columns of the input CSR (seeds are the playlist's own tracks).  -> (seed_row_ptr, seed_col)."""
        import torch
        B = row_ptr.numel() - 1
        srp = torch.empty(B + 1, dtype=torch.int32, device=row_ptr.device)
        sc = torch.empty(max(int(col.numel()), 1), dtype=torch.int32, device=row_ptr.device)
        self.check(self.lib.dae_seeds_from_csr(self.h, _ptr(row_ptr), _ptr(col), B, int(n_tracks), _ptr(srp), _ptr(sc)))
        return srp, sc

    def train_batch(self, train_set, draw, x_side, x_cap, y_cap):
        """Both CSRs of a training step from the reader's draws (dae_train_batch).  draw: int32 [3, B] CUDA tensor (playlist
        index, given tracks, given artists); x_side 0 tracks / 1 artists / 2 both; x_cap / y_cap: room of the outputs in
        entries (an upper bound of the kept entries).  -> ((x_row_ptr, x_col, x_val), (y_row_ptr, y_col, y_val), status):
        status bit 0 = a playlist index out of range, bit 1 = a capacity was too small."""
        import torch
        B = int(draw.shape[1])
        assert draw.dtype == torch.int32 and draw.is_contiguous() and draw.shape[0] == 3
        dev = draw.device
        out = []
        for cap in (x_cap, y_cap):
            out.append((torch.empty(B + 1, dtype=torch.int32, device=dev), torch.empty(max(int(cap), 1), dtype=torch.int32, device=dev),
                        torch.empty(max(int(cap), 1), dtype=torch.float32, device=dev)))
        status = torch.empty(1, dtype=torch.int32, device=dev)
        (xr, xc, xv), (yr, yc, yv) = out
        self.check(self.lib.dae_train_batch(self.h, train_set.h, _ptr(draw), B, int(x_side), _ptr(xr), _ptr(xc), _ptr(xv),
                                            int(x_cap), _ptr(yr), _ptr(yc), _ptr(yv), int(y_cap), _ptr(status)))
        return out[0], out[1], status

    def train_titles(self, train_set, draw):
        """The title rows of a drawn batch (dae_train_titles; the set holds titles: TrainSet.attach_titles).  draw: the int32
        [3, B] CUDA tensor `train_batch` takes.  -> int32 [B, L] CUDA tensor; a playlist index out of range gives a row of -1
        (and `train_batch`'s status bit 0 for the same draw)."""
        import torch
        assert draw.dtype == torch.int32 and draw.is_contiguous() and draw.shape[0] == 3
        B = int(draw.shape[1])
        out = torch.empty((B, max(int(train_set.title_len), 1)), dtype=torch.int32, device=draw.device)
        self.check(self.lib.dae_train_titles(self.h, train_set.h, _ptr(draw), B, _ptr(out)))
        return out

    def set_train_dtype(self, dtype):
        """Arithmetic of the training forward GEMM: DAE_DTYPE_F32 (default) or DAE_DTYPE_BF16."""
        self.check(self.lib.dae_set_train_dtype(self.h, int(dtype)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.dae_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- thin wrappers (torch CUDA tensors in, results written into caller tensors) ------------
    def encode(self, row_ptr, col, val, W_enc, b_enc, h_out, ikp=1.0, kp=1.0, seed=0):
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        self.check(self.lib.dae_encode(self.h, _ptr(row_ptr), _ptr(col), _ptr(val), _ptr(W_enc),
                                       _ptr(b_enc), V, H, B, float(ikp), float(kp),
                                       int(seed) & 0xFFFFFFFF, _ptr(h_out)))

    def prepack_decoder(self, W_dec, b_dec, col_lo=0, col_hi=None, dtype=DAE_DTYPE_F32):
        V, H = W_dec.shape
        if col_hi is None:
            col_hi = V
        self.check(self.lib.dae_prepack_decoder(self.h, _ptr(W_dec), _ptr(b_dec), V, H,
                                                int(col_lo), int(col_hi), int(dtype)))
        self._drop_share(dtype)

    @staticmethod
    def _slot(dtype):
        return "f32" if int(dtype) == DAE_DTYPE_F32 else "bf16"      # the two image slots of a context (dae_packed)

    def _drop_share(self, dtype):
        """The slot holds an image of its own again: the context it borrowed from need not be kept alive for it."""
        self.__dict__.setdefault("_shares", {}).pop(self._slot(dtype), None)

    def prepack_decoder_rows(self, W_rows, b_rows, col_lo, dtype=DAE_DTYPE_F32):
        """Prepack a decoder image from a RANK-LOCAL copy of its rows: W_rows [n, H] / b_rows [n] hold the global
        columns col_lo .. col_lo + n (dae_prepack_decoder_rows)."""
        n, H = W_rows.shape
        assert W_rows.is_contiguous() and b_rows.is_contiguous() and b_rows.numel() == n
        self.check(self.lib.dae_prepack_decoder_rows(self.h, _ptr(W_rows), _ptr(b_rows), int(n), H, int(col_lo), int(dtype)))
        self._drop_share(dtype)

    def title_loss_backward_cols(self, z_title, dae_score, y_csr, w_title, w_playlist, col_lo, col_hi, n_batch, feat,
                                 Output_WT_rows, gOutput_WT_rows, gOutput_b_rows, dfeat_partial, cost_partial):
        """The title loss head and the output layer's gradients on the vocabulary columns [col_lo, col_hi)
        (dae_title_loss_backward_cols): z_title / dae_score [B, col_hi - col_lo], y_csr the WHOLE batch's (row_ptr, col,
        val) with global ids, the *_rows tensors the rows col_lo .. col_hi of their arrays; dfeat_partial [B, ld] and
        cost_partial [1] receive this window's addends."""
        B, ld = feat.shape
        self.check(self.lib.dae_title_loss_backward_cols(
            self.h, _ptr(z_title), int(z_title.stride(0)), _ptr(dae_score), int(dae_score.stride(0)),
            _ptr(y_csr[0]), _ptr(y_csr[1]), _ptr(y_csr[2]), _ptr(w_title), _ptr(w_playlist), int(B), int(col_lo), int(col_hi),
            int(n_batch), _ptr(feat), int(ld), _ptr(Output_WT_rows), _ptr(gOutput_WT_rows), _ptr(gOutput_b_rows),
            _ptr(dfeat_partial), _ptr(cost_partial)))

    def set_overlap_hint(self, batches_in_flight):
        """Other batches are in flight on other streams: kernel shapes that share CUs (include/dae_hip.h)."""
        self.check(self.lib.dae_set_overlap_hint(self.h, int(batches_in_flight)))

    def share_decoder(self, src, dtype=DAE_DTYPE_F32):
        """Use `src`'s prepacked image of `dtype` instead of an own copy (see include/dae_hip.h dae_share_decoder: `src`
        outlives every use; order src's prepack before this context's first launch)."""
        self.check(self.lib.dae_share_decoder(self.h, src.h, int(dtype)))
        self.__dict__.setdefault("_shares", {})[self._slot(dtype)] = src     # one owner per slot, alive while borrowed

    def exact_bounds(self, eps_out):
        """Per-column bounds |fp32 logit - bf16 logit| <= eps of the image prepacked with DAE_DTYPE_BF16_EXACT."""
        self.check(self.lib.dae_exact_bounds(self.h, _ptr(eps_out)))

    def set_exact_margin(self, scale):
        """Factor on every eps_c at the NEXT exact prepack (include/dae_hip.h: > 1 widens, < 1 voids the bound -- the
        guard's test hook)."""
        self.check(self.lib.dae_set_exact_margin(self.h, float(scale)))
        self._exact_margin = float(scale)        # (models/DAEs.py hands it on to the pipelines it builds from this model)

    def set_exact_margin_range(self, col_from, col_to, scale):
        """The same for the columns [col_from, col_to) alone (the audit's test hook: a column every row drops)."""
        self.check(self.lib.dae_set_exact_margin_range(self.h, int(col_from), int(col_to), float(scale)))

    def set_exact_audit(self, every_n, n_tiles=16):
        """Every every_n-th exact scoring launch audits n_tiles random tiles of DROPPED columns (0: never; include/dae_hip.h)."""
        self.check(self.lib.dae_set_exact_audit(self.h, int(every_n), int(n_tiles)))

    def exact_audit_read(self):
        """{audits, checked, violations} of the dropped-column audit since the context was created (synchronises)."""
        a = (ctypes.c_uint64 * 3)()
        self.check(self.lib.dae_exact_audit_read(self.h, a))
        return {"audits": int(a[0]), "checked": int(a[1]), "violations": int(a[2])}

    def exact_guard_read(self):
        """(violations, column) of the exact mode's bound guard since the last non-zero read; synchronises the stream."""
        n, c = ctypes.c_int32(), ctypes.c_int32()
        self.check(self.lib.dae_exact_guard_read(self.h, ctypes.byref(n), ctypes.byref(c)))
        if n.value:
            self._guard_seen = 0             # (the read reset the cumulative words: snapshots compare against zero again)
        return int(n.value), int(c.value)

    def guard_moved(self, n_bad):
        """A launch's snapshot against the previous one taken on this context: True when the count changed under it."""
        seen = getattr(self, "_guard_seen", 0)
        self._guard_seen = int(n_bad)
        return int(n_bad) != seen

    def exact_stats_read(self):
        """{rows, candidates_per_row, recomputed_per_row} of the refine launches since the last read (synchronises)."""
        a = (ctypes.c_uint64 * 3)()
        self.check(self.lib.dae_exact_stats_read(self.h, a))
        rows = max(int(a[0]), 1)
        return {"rows": int(a[0]), "candidates_per_row": round(int(a[1]) / rows, 1), "recomputed_per_row": round(int(a[2]) / rows, 1)}

    def set_filter_skip(self, on=True):
        """The fp32 hidden-256 filter launch walks only the tiles whose logit bound reaches the threshold (default on;
        include/dae_hip.h).  Off: every planned tile -- the same lists and scores."""
        self.check(self.lib.dae_set_filter_skip(self.h, 1 if on else 0))

    def filter_skip_read(self):
        """{launches, planned, live} filter tiles (summed over row groups) since the last read; resets; synchronises."""
        a = (ctypes.c_uint64 * 3)()
        self.check(self.lib.dae_filter_skip_read(self.h, a))
        return {"launches": int(a[0]), "planned": int(a[1]), "live": int(a[2])}

    def sample_skip_read(self):
        """{launches, planned, decoded} wave-tiles of the threshold samples that could skip tiles by their bound (half row
        groups: include/dae_hip.h) since the last read; resets; synchronises."""
        a = (ctypes.c_uint64 * 3)()
        self.check(self.lib.dae_sample_skip_read(self.h, a))
        return {"launches": int(a[0]), "planned": int(a[1]), "decoded": int(a[2])}

    def live_proof_read(self):
        """Row groups whose live list the threshold launch proved empty (no hand-off between the rows' workgroups:
        include/dae_hip.h) since the last read; resets; synchronises."""
        a = ctypes.c_uint64(0)
        self.check(self.lib.dae_live_proof_read(self.h, ctypes.byref(a)))
        return int(a.value)

    def last_tau(self, B):
        """The thresholds of the context's last score_topk / decode_topk as a float32 array [B] (dae_last_tau_read); synchronises."""
        import numpy as np
        out = np.empty(B, np.float32)
        self.check(self.lib.dae_last_tau_read(self.h, out.ctypes.data_as(ctypes.c_void_p), int(B)))
        return out

    def filter_skip_last(self):
        """Live filter tiles per row group of the context's last ranking call ([] when it built no live lists); synchronises."""
        a, n = (ctypes.c_int32 * 64)(), ctypes.c_int()
        self.check(self.lib.dae_filter_skip_last(self.h, a, 64, ctypes.byref(n)))
        return [int(a[i]) for i in range(min(n.value, 64))]

    def tile_bounds(self):
        """The fp32 image's per-tile logit bounds as a float32 array [ntiles, 2] = (A_t, M_t) (include/dae_hip.h); synchronises."""
        import numpy as np
        n = ctypes.c_int()
        self.check(self.lib.dae_tile_bounds_read(self.h, None, 0, ctypes.byref(n)))
        out = np.empty((max(n.value, 1), 2), np.float32)
        self.check(self.lib.dae_tile_bounds_read(self.h, out.ctypes.data_as(ctypes.c_void_p), n.value, ctypes.byref(n)))
        return out[:n.value]

    def decode_dense(self, h, out, apply_sigmoid=True, dtype=DAE_DTYPE_F32):
        B, H = h.shape
        self.check(self.lib.dae_decode_dense(self.h, _ptr(h), B, H, int(dtype),
                                             1 if apply_sigmoid else 0, _ptr(out),
                                             int(out.stride(0))))

    def decode_loss_rows(self, h, y_csr, W_dec, b_dec, row_loss, dtype=DAE_DTYPE_F32):
        """row_loss[r] = the loss of row r of the hidden rows h [B, H] over all V columns against the target CSR y_csr =
        (row_ptr, col, val), over the context's prepacked image of `dtype` (dae_decode_loss_rows; nothing per element is
        stored)."""
        B, H = h.shape
        V = W_dec.shape[0]
        self.check(self.lib.dae_decode_loss_rows(self.h, _ptr(h), B, H, int(dtype), _ptr(y_csr[0]), _ptr(y_csr[1]), _ptr(y_csr[2]),
                                                 _ptr(W_dec), _ptr(b_dec), int(V), _ptr(row_loss)))

    def score_loss(self, x_csr, y_csr, W_enc, b_enc, W_dec, b_dec, n_batch, tied, ikp=1.0, kp=1.0, seed=0, reg_lambda=0.0,
                   row_loss=None, cost_out=None):
        """The cost of a batch without a step (dae_score_loss): the step's encode with its dropout masks, the loss of every
        row into row_loss [B] and / or cost_out [1] = sum(row_loss) / n_batch + reg_lambda * l2 (CUDA tensors; either may be
        None).  The image of the context's train dtype must be current (prepack_decoder)."""
        V, H = W_enc.shape
        B = x_csr[0].numel() - 1
        self.check(self.lib.dae_score_loss(
            self.h, _ptr(x_csr[0]), _ptr(x_csr[1]), _ptr(x_csr[2]), _ptr(y_csr[0]), _ptr(y_csr[1]), _ptr(y_csr[2]),
            _ptr(W_enc), _ptr(b_enc), _ptr(W_dec) if W_dec is not None else None, _ptr(b_dec), int(V), int(H), int(B),
            int(n_batch), 1 if tied else 0, float(ikp), float(kp), int(seed) & 0xFFFFFFFF, float(reg_lambda),
            _ptr(row_loss) if row_loss is not None else None, _ptr(cost_out) if cost_out is not None else None))

    def decode_topk(self, h, n_tracks, seed_row_ptr, seed_col, k, out_score, out_idx,
                    out_kind=DAE_OUT_SCORE, dtype=DAE_DTYPE_F32):
        B, H = h.shape
        self.check(self.lib.dae_decode_topk(self.h, _ptr(h), B, H, int(dtype), int(n_tracks),
                                            _ptr(seed_row_ptr), _ptr(seed_col), int(k),
                                            int(out_kind), _ptr(out_score), _ptr(out_idx)))

    def score_topk(self, row_ptr, col, val, W_enc, b_enc, n_tracks, seed_row_ptr, seed_col, k,
                   out_score, out_idx, out_kind=DAE_OUT_SCORE, dtype=DAE_DTYPE_F32):
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        self.check(self.lib.dae_score_topk(self.h, _ptr(row_ptr), _ptr(col), _ptr(val),
                                           _ptr(W_enc), _ptr(b_enc), V, H, B, int(dtype),
                                           int(n_tracks), _ptr(seed_row_ptr), _ptr(seed_col),
                                           int(k), int(out_kind), _ptr(out_score), _ptr(out_idx)))

    def score_topk_handle(self, row_ptr, col, val, W_enc, b_enc, n_tracks, seed_row_ptr, seed_col, k,
                          out_score, out_idx, out_kind=DAE_OUT_SCORE, dtype=DAE_DTYPE_F32):
        """`score_topk` with its arguments marshalled ONCE: returns a zero-argument callable that enqueues the call on
        the context's stream (a driver that scores resident batches issues one every ~30 us: building 17 ctypes
        arguments and a torch stream context per call was a third of that).  The tensors must stay alive and in place."""
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        args = (self.h, _ptr(row_ptr), _ptr(col), _ptr(val), _ptr(W_enc), _ptr(b_enc), V, H, B, int(dtype), int(n_tracks),
                _ptr(seed_row_ptr), _ptr(seed_col), int(k), int(out_kind), _ptr(out_score), _ptr(out_idx))
        fn, check = self.lib.dae_score_topk, self.check
        keep = (row_ptr, col, val, W_enc, b_enc, seed_row_ptr, seed_col, out_score, out_idx)

        def call(_keep=keep):
            rc = fn(*args)
            if rc:
                check(rc)
        return call

    def score_topk_begin(self, row_ptr, col, val, W_enc, b_enc, n_tracks, seed_row_ptr, k, tau_out, dtype=DAE_DTYPE_F32):
        """First half of score_topk: encode + threshold sample -> tau_out [B] (this image's per-row lower bounds)."""
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        self.check(self.lib.dae_score_topk_begin(self.h, _ptr(row_ptr), _ptr(col), _ptr(val), _ptr(W_enc), _ptr(b_enc),
                                                 V, H, B, int(dtype), int(n_tracks), _ptr(seed_row_ptr), int(k),
                                                 _ptr(tau_out)))

    def score_topk_finish(self, tau, seed_row_ptr, seed_col, out_score, out_idx, out_kind=DAE_OUT_SCORE):
        """Second half: filter with `tau` [B] (the own bounds or the maximum over the shards) + selection."""
        self.check(self.lib.dae_score_topk_finish(self.h, _ptr(tau), _ptr(seed_row_ptr), _ptr(seed_col), int(out_kind),
                                                  _ptr(out_score), _ptr(out_idx)))

    def topk_dense(self, logits, ncols, col_base, seed_row_ptr, seed_col, k, out_score, out_idx,
                   out_kind=DAE_OUT_SCORE):
        B = logits.shape[0]
        ld = int(logits.stride(0)) if B > 1 else max(int(logits.stride(0)), int(logits.shape[1]))   # a 1-row view may carry stride 0
        self.check(self.lib.dae_topk_dense(self.h, _ptr(logits), ld, B,
                                           int(ncols), int(col_base), _ptr(seed_row_ptr),
                                           _ptr(seed_col), int(k), int(out_kind),
                                           _ptr(out_score), _ptr(out_idx)))

    def decode_mix_term(self, h, row_scale, n_cols, outT, dtype=DAE_DTYPE_F32):
        """outT[c, r] = row_scale[r] * sigmoid(logit[r, c]) for the prepacked columns c < n_cols (DAEs.py:180, DAE term)."""
        B, H = h.shape
        self.check(self.lib.dae_decode_mix_term(self.h, _ptr(h), B, H, int(dtype), _ptr(row_scale), int(n_cols),
                                                _ptr(outT), int(outT.stride(0))))

    def decode_mix_term_add(self, h, row_scale, n_cols, accT, dtype=DAE_DTYPE_F32):
        """accT[c, r] = accT[c, r] + row_scale[r] * sigmoid(logit[r, c]) for the prepacked columns c < n_cols: a further member's
        term of an ensemble, added to the buffer `decode_mix_term` wrote (dae_decode_mix_term_add)."""
        B, H = h.shape
        self.check(self.lib.dae_decode_mix_term_add(self.h, _ptr(h), B, H, int(dtype), _ptr(row_scale), int(n_cols),
                                                    _ptr(accT), int(accT.stride(0))))

    def set_score_mix(self, mixT=None, w_title=None):
        """dae_decode_topk on this context ranks sigmoid(.) * w_title[r] + mixT[c, r] until cleared (no arguments)."""
        self.check(self.lib.dae_set_score_mix(self.h, _ptr(mixT), int(mixT.stride(0)) if mixT is not None else 0,
                                              int(mixT.shape[0]) if mixT is not None else 0, _ptr(w_title)))

    def ensemble_topk(self, members, hs, row_scales, n_tracks, seed_row_ptr, seed_col, k, out_score, out_idx,
                      dtype=DAE_DTYPE_F32, feat=None, w_title=None):
        """On the RANKING context of an ensemble -- the title scorer's when feat / w_title are given, else the last member's:
        the top-k of the members' weighted sigmoids summed in the order include/dae_hip.h fixes (dae_ensemble_topk).  members:
        their contexts, this one last when untitled; hs / row_scales: per member its hidden rows [B, H_m] and weights [B]."""
        M = len(members)
        if M < 1 or len(hs) != M or len(row_scales) != M:
            raise ValueError("ensemble_topk: one hidden-row tensor and one weight vector per member")
        titled = feat is not None
        if not titled and members[-1] is not self:
            raise ValueError("ensemble_topk: untitled, the last member's context ranks -- call it on that context")
        vp = ctypes.c_void_p
        B = int(hs[0].shape[0])
        for t in list(hs) + list(row_scales) + ([feat] if titled else []):
            if t is not None and not t.is_contiguous():
                raise ValueError("ensemble_topk: contiguous tensors are required")
        c_m = (vp * M)(*[m.h for m in members])
        c_h = (vp * M)(*[vp(t.data_ptr()) if t is not None else None for t in hs])
        c_H = (ctypes.c_int * M)(*[int(t.shape[1]) if t is not None else 0 for t in hs])
        c_a = (vp * M)(*[vp(t.data_ptr()) if t is not None else None for t in row_scales])
        self.check(self.lib.dae_ensemble_topk(c_m, M, c_h, c_H, c_a, self.h if titled else None, _ptr(feat),
                                              int(feat.shape[1]) if titled else 0, _ptr(w_title), B, int(dtype), int(n_tracks),
                                              _ptr(seed_row_ptr), _ptr(seed_col), int(k), _ptr(out_score), _ptr(out_idx)))

    def _ensemble_args(self, name, members, hs, row_scales, W_decs, b_decs, feat, OutW_T, Out_b, w_title):
        """The scorers of an ensemble call as the C ABI takes them (dae_ensemble_candidates / dae_ensemble_rank_of), this context
        being the ranking one."""
        M = len(members)
        if M < 1 or not (len(hs) == len(row_scales) == len(W_decs) == len(b_decs) == M):
            raise ValueError("%s: one hidden-row tensor, weight vector, decoder tensor and bias per member" % name)
        titled = feat is not None
        if not titled and members[-1] is not self:
            raise ValueError("%s: untitled, the last member's context ranks -- call it on that context" % name)
        for t in list(hs) + list(row_scales) + list(W_decs) + list(b_decs) + ([feat, OutW_T] if titled else []):
            if t is not None and not t.is_contiguous():
                raise ValueError("%s: contiguous tensors are required" % name)
        vp = ctypes.c_void_p
        arr = lambda ts: (vp * M)(*[vp(t.data_ptr()) if t is not None else None for t in ts])      # noqa: E731
        c_H = (ctypes.c_int * M)(*[int(t.shape[1]) if t is not None else 0 for t in hs])
        return ((vp * M)(*[m.h for m in members]), M, arr(hs), c_H, arr(row_scales), arr(W_decs), arr(b_decs),
                self.h if titled else None, _ptr(feat), int(feat.shape[1]) if titled else 0, _ptr(OutW_T), _ptr(Out_b),
                _ptr(w_title), int(hs[0].shape[0]), int(W_decs[0].shape[0]))

    def ensemble_candidates(self, members, hs, row_scales, W_decs, b_decs, cand, n_cand, out, feat=None, OutW_T=None, Out_b=None,
                            w_title=None, status=None):
        """On the RANKING context of an ensemble (as ensemble_topk): out[i] = the canonical value y of column cand_col[i] for its
        row (dae_ensemble_candidates).  W_decs / b_decs: per member its row-major decoder tensor [V, H_m] and bias [V]."""
        args = self._ensemble_args("ensemble_candidates", members, hs, row_scales, W_decs, b_decs, feat, OutW_T, Out_b, w_title)
        self.check(self.lib.dae_ensemble_candidates(*args, _ptr(cand[0]), _ptr(cand[1]), int(n_cand), _ptr(out), _ptr(status)))

    def ensemble_rank_of(self, members, hs, row_scales, W_decs, b_decs, n_tracks, seed_row_ptr, seed_col, ans, n_ans, out_rank,
                         out_score=None, feat=None, OutW_T=None, Out_b=None, w_title=None, status=None, n_seed=None):
        """On the RANKING context of an ensemble: decode_rank_of under the ensemble's y (dae_ensemble_rank_of).  Every context
        holds its plain fp32 image over all columns.  n_seed: the length of seed_col by default."""
        args = self._ensemble_args("ensemble_rank_of", members, hs, row_scales, W_decs, b_decs, feat, OutW_T, Out_b, w_title)
        if n_seed is None:
            n_seed = int(seed_col.numel()) if seed_col is not None else 0
        self.check(self.lib.dae_ensemble_rank_of(*args, int(n_tracks), _ptr(seed_row_ptr), _ptr(seed_col), int(n_seed),
                                                 _ptr(ans[0]), _ptr(ans[1]), int(n_ans), _ptr(out_rank), _ptr(out_score),
                                                 _ptr(status)))

    def mix_topk_exact(self, dae_ctx, feat, h, w_title, w_playlist, n_tracks, seed_row_ptr, seed_col, k, out_score, out_idx,
                       guard_out=None):
        """On the title scorer's context: top-k of the title mix, bit-identical to the fp32 path, both GEMMs on bf16
        operands (dae_mix_topk_exact; both contexts prepacked with DAE_DTYPE_BF16_EXACT and bound to the same stream)."""
        B = h.shape[0]
        self.check(self.lib.dae_mix_topk_exact(self.h, dae_ctx.h, _ptr(feat), int(feat.stride(0)), _ptr(h), int(h.stride(0)),
                                               int(B), _ptr(w_title), _ptr(w_playlist), int(n_tracks), _ptr(seed_row_ptr),
                                               _ptr(seed_col), int(k), _ptr(out_score), _ptr(out_idx), _ptr(guard_out)))

    # ---- caller-given candidate columns (csrc/candidates.hip): cand = (row_ptr int32 [B + 1], col int32 [>= n_cand]) ----------
    def decode_candidates(self, h, W_dec, b_dec, cand, n_cand, out, out_kind=DAE_OUT_SCORE, status=None):
        """out[i] = score or logit of column cand_col[i] for its row's hidden row (dae_decode_candidates)."""
        B, H = h.shape
        self.check(self.lib.dae_decode_candidates(self.h, _ptr(h), int(h.stride(0)), B, H, _ptr(W_dec), _ptr(b_dec),
                                                  int(W_dec.shape[0]), _ptr(cand[0]), _ptr(cand[1]), int(n_cand), int(out_kind),
                                                  _ptr(out), _ptr(status)))

    def score_candidates(self, row_ptr, col, val, W_enc, b_enc, W_dec, b_dec, cand, n_cand, out, out_kind=DAE_OUT_SCORE,
                         status=None):
        """dae_encode (inference) + decode_candidates in one call; the hidden rows stay in the context."""
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        self.check(self.lib.dae_score_candidates(self.h, _ptr(row_ptr), _ptr(col), _ptr(val), _ptr(W_enc), _ptr(b_enc), V, H, B,
                                                 _ptr(W_dec), _ptr(b_dec), _ptr(cand[0]), _ptr(cand[1]), int(n_cand),
                                                 int(out_kind), _ptr(out), _ptr(status)))

    def mix_candidates(self, dae_ctx, h, W_dec, b_dec, feat, OutW_T, Out_b, w_title, w_playlist, cand, n_cand, out, status=None):
        """On the title scorer's context: the title-mixed score of the listed (row, column) pairs (dae_mix_candidates)."""
        B, H = h.shape
        self.check(self.lib.dae_mix_candidates(self.h, dae_ctx.h, _ptr(h), int(h.stride(0)), H, _ptr(W_dec), _ptr(b_dec), _ptr(feat),
                                               int(feat.stride(0)), _ptr(OutW_T), _ptr(Out_b), _ptr(w_title), _ptr(w_playlist),
                                               B, int(W_dec.shape[0]), _ptr(cand[0]), _ptr(cand[1]), int(n_cand), _ptr(out),
                                               _ptr(status)))

    def rank_candidates(self, n_cols, cand, key, row_cap, seed_row_ptr, seed_col, k, out_score, out_idx, out_kind=DAE_OUT_SCORE):
        """The k best candidates of every row by `key` (dae_rank_candidates); row_cap >= the longest row."""
        B = cand[0].numel() - 1
        self.check(self.lib.dae_rank_candidates(self.h, B, int(n_cols), _ptr(cand[0]), _ptr(cand[1]), _ptr(key), int(row_cap),
                                                _ptr(seed_row_ptr), _ptr(seed_col), int(k), int(out_kind), _ptr(out_score),
                                                _ptr(out_idx)))

    def candidates_unique(self, n_cols, cand, n_cand, out=None):
        """Per row, every repeated column but one -> -1 (dae_candidates_unique); out=None: in place."""
        B = cand[0].numel() - 1
        self.check(self.lib.dae_candidates_unique(self.h, B, int(n_cols), _ptr(cand[0]), _ptr(cand[1]),
                                                  _ptr(cand[1] if out is None else out), int(n_cand)))

    # ---- exact ranks of given tracks over the whole vocabulary (csrc/rank_of.hip): ans = (row_ptr int32 [B + 1], col int32 [>= n_ans])
    def decode_rank_of(self, h, W_dec, b_dec, n_tracks, seed_row_ptr, seed_col, ans, n_ans, out_rank, out_logit=None, status=None):
        """out_rank[i] = how many rankable non-seed tracks precede column ans_col[i] in its row's canonical fp32 order, -1 for
        what cannot be ranked (dae_decode_rank_of); needs the plain fp32 image of W_dec / b_dec over all columns."""
        B, H = h.shape
        if not h.is_contiguous():
            raise ValueError("decode_rank_of: contiguous hidden rows are required")
        self.check(self.lib.dae_decode_rank_of(self.h, _ptr(h), B, H, _ptr(W_dec), _ptr(b_dec), int(W_dec.shape[0]), int(n_tracks),
                                               _ptr(seed_row_ptr), _ptr(seed_col), _ptr(ans[0]), _ptr(ans[1]), int(n_ans),
                                               _ptr(out_rank), _ptr(out_logit), _ptr(status)))

    def score_rank_of(self, row_ptr, col, val, W_enc, b_enc, W_dec, b_dec, n_tracks, seed_row_ptr, seed_col, ans, n_ans, out_rank,
                      out_logit=None, status=None):
        """dae_encode (inference) + decode_rank_of in one call; the hidden rows stay in the context."""
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        self.check(self.lib.dae_score_rank_of(self.h, _ptr(row_ptr), _ptr(col), _ptr(val), _ptr(W_enc), _ptr(b_enc), V, H, B,
                                              _ptr(W_dec), _ptr(b_dec), int(n_tracks), _ptr(seed_row_ptr), _ptr(seed_col),
                                              _ptr(ans[0]), _ptr(ans[1]), int(n_ans), _ptr(out_rank), _ptr(out_logit),
                                              _ptr(status)))

    def mix_rank_of(self, dae_ctx, h, W_dec, b_dec, feat, OutW_T, Out_b, w_title, w_playlist, n_tracks, seed_row_ptr, seed_col, ans,
                    n_ans, out_rank, out_score=None, status=None):
        """On the title scorer's context: decode_rank_of under the title mix -- the ranks by y = sigmoid(z_title) * w_title +
        sigmoid(z_dae) * w_playlist, out_score = y (dae_mix_rank_of).  Both contexts hold their plain fp32 image over all
        columns and are bound to one stream; h [B, H] contiguous."""
        B, H = h.shape
        if not (h.is_contiguous() and feat.is_contiguous()):
            raise ValueError("mix_rank_of: contiguous hidden and feature rows are required")
        self.check(self.lib.dae_mix_rank_of(self.h, dae_ctx.h, _ptr(h), H, H, _ptr(W_dec),
                                            _ptr(b_dec), _ptr(feat), int(feat.shape[1]), _ptr(OutW_T), _ptr(Out_b), _ptr(w_title),
                                            _ptr(w_playlist), B, int(W_dec.shape[0]), int(n_tracks), _ptr(seed_row_ptr),
                                            _ptr(seed_col), _ptr(ans[0]), _ptr(ans[1]), int(n_ans), _ptr(out_rank),
                                            _ptr(out_score), _ptr(status)))

    def mix_loss_rows(self, dae_ctx, h, W_dec, b_dec, feat, OutW_T, Out_b, w_title, w_playlist, n_batch, y_csr, row_loss=None,
                      cost_out=None):
        """On the title scorer's context: the loss of the MIXED score without a step (dae_mix_loss_rows) -- the loss of every
        row of h [B, H] / feat [B, ld_feat] over all V columns against the target CSR y_csr = (row_ptr, col, val) into row_loss
        [B] and / or cost_out [1] = sum(row_loss) / n_batch (CUDA tensors; either may be None).  Both contexts hold their plain
        fp32 image over all columns and are bound to one stream."""
        B, H = h.shape
        if not (h.is_contiguous() and feat.is_contiguous()):
            raise ValueError("mix_loss_rows: contiguous hidden and feature rows are required")
        self.check(self.lib.dae_mix_loss_rows(
            self.h, dae_ctx.h, _ptr(h), H, H, _ptr(W_dec), _ptr(b_dec), _ptr(feat), int(feat.shape[1]), _ptr(OutW_T), _ptr(Out_b),
            _ptr(w_title), _ptr(w_playlist), B, int(W_dec.shape[0]), int(n_batch), _ptr(y_csr[0]), _ptr(y_csr[1]), _ptr(y_csr[2]),
            _ptr(row_loss) if row_loss is not None else None, _ptr(cost_out) if cost_out is not None else None))

    # ---- a catalogue: a shared, ascending subset of the track columns (csrc/catalogue.hip; `Catalogue` below) ------------------
    def prepack_decoder_catalogue(self, cat, W_dec, b_dec, dtype=DAE_DTYPE_F32):
        """This context's image of `dtype` from rows cat.columns of W_dec [V, H] / b_dec [V] (dae_prepack_decoder_catalogue): local
        columns [0, n).  The gathered copy is a temporary of the call."""
        V, H = W_dec.shape
        assert W_dec.is_contiguous() and b_dec.is_contiguous() and b_dec.numel() == V
        self.check(self.lib.dae_prepack_decoder_catalogue(self.h, cat.h, _ptr(W_dec), _ptr(b_dec), int(V), int(H), int(dtype)))
        self._drop_share(dtype)

    def score_topk_catalogue(self, cat, row_ptr, col, val, W_enc, b_enc, seed_row_ptr, seed_col, k, out_score, out_idx,
                             out_kind=DAE_OUT_SCORE, dtype=DAE_DTYPE_F32):
        """`score_topk` over the catalogue's columns (dae_score_topk_catalogue): seeds and out_idx are GLOBAL columns."""
        V, H = W_enc.shape
        B = row_ptr.numel() - 1
        n_seeds = int(seed_col.numel()) if seed_col is not None else 0
        self.check(self.lib.dae_score_topk_catalogue(self.h, _ptr(row_ptr), _ptr(col), _ptr(val), _ptr(W_enc), _ptr(b_enc), V, H, B,
                                                     int(dtype), cat.h, _ptr(seed_row_ptr), _ptr(seed_col), n_seeds, int(k),
                                                     int(out_kind), _ptr(out_score), _ptr(out_idx)))

    def decode_topk_catalogue(self, cat, h, seed_row_ptr, seed_col, k, out_score, out_idx, out_kind=DAE_OUT_SCORE,
                              dtype=DAE_DTYPE_F32):
        """`decode_topk` over the catalogue's columns (dae_decode_topk_catalogue)."""
        B, H = h.shape
        n_seeds = int(seed_col.numel()) if seed_col is not None else 0
        self.check(self.lib.dae_decode_topk_catalogue(self.h, _ptr(h), B, H, int(dtype), cat.h, _ptr(seed_row_ptr), _ptr(seed_col),
                                                      n_seeds, int(k), int(out_kind), _ptr(out_score), _ptr(out_idx)))

    def title_score_catalogue(self, cat, dae_ctx, dtype, positions, values, n_rows, W_enc, b_enc, titles, emb, n_char, conv_w,
                              conv_b, filter_sizes, F, ld_feat, titles_use, n_tracks, k, out_score, out_idx, csr_status,
                              guard_out=None):
        """On the title scorer's context: one titled launch over the catalogue's columns (dae_title_score_catalogue).  positions
        int64 [nnz, 2] / values float32 [nnz] or [1]: the feed on the device; titles int32 [n_rows, L]; filter_sizes a ctypes
        int32 array.  Both contexts hold images gathered from `cat`."""
        V, H = W_enc.shape
        nnz = int(positions.shape[0])
        bcast = 1 if (values.numel() == 1 and nnz != 1) else 0
        self.check(self.lib.dae_title_score_catalogue(
            self.h, dae_ctx.h, int(dtype), _ptr(positions), _ptr(values), bcast, nnz, int(n_rows), int(V), _ptr(W_enc), _ptr(b_enc),
            int(H), _ptr(titles), int(titles.shape[1]), _ptr(emb), int(n_char), int(emb.shape[1]), _ptr(conv_w), _ptr(conv_b),
            filter_sizes, len(filter_sizes), int(F), int(ld_feat), _ptr(titles_use), int(n_tracks), int(k), _ptr(out_score),
            _ptr(out_idx), _ptr(guard_out), _ptr(csr_status), cat.h))

    def topk_merge(self, cand_logit, cand_idx, out_score, out_idx, out_kind=DAE_OUT_SCORE):
        G, B, k = cand_logit.shape
        self.check(self.lib.dae_topk_merge(self.h, G, B, k, _ptr(cand_logit), _ptr(cand_idx),
                                           int(out_kind), _ptr(out_score), _ptr(out_idx)))

    def rank_metrics(self, idx, k, ans_row_ptr, ans_col, out=None, disc=None):
        """dae_rank_metrics: idx int32 [B, ld >= k], the answers as a CSR (int32 CUDA tensors) -> a uint8 CUDA tensor [B, 24]
        holding one dae_metric_rec per row (`.cpu().numpy().view(metrics.RECORD_DTYPE)`).  disc: float64 [k] CUDA tensor,
        by default Python's own 1 / math.log(p + 1, 2) (utils/metrics.py discount_table)."""
        import torch
        B, ld = int(idx.shape[0]), int(idx.stride(0)) if idx.dim() == 2 else int(k)
        if disc is None:
            from .utils.metrics import discount_table
            disc = torch.from_numpy(discount_table(k)).to(idx.device)
        if out is None:
            out = torch.empty((B, 24), dtype=torch.uint8, device=idx.device)
        self.check(self.lib.dae_rank_metrics(self.h, _ptr(idx), ld, B, int(k), _ptr(ans_row_ptr), _ptr(ans_col), _ptr(disc),
                                             _ptr(out)))
        return out

    def profile_enable(self, on=True):
        self.check(self.lib.dae_profile_enable(self.h, 1 if on else 0))

    def profile_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_int()
        self.check(self.lib.dae_profile_read(self.h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_kernel(self):
        """Symbol of the kernel the last profiled launch ran (what rocprofv3's kernel trace calls it)."""
        return self.lib.dae_profile_kernel(self.h).decode()

    def clock_probe(self, out2, stream=None, window_us=50):
        """Enqueue the one-wave clock sampler (`out2`: CUDA int64/uint64 tensor of 2); returns the wall clock's kHz.
        GHz = out2[0] / out2[1] * kHz / 1e6 once the stream has run it."""
        khz = ctypes.c_int()
        self.check(self.lib.dae_clock_probe(self.h, ctypes.c_void_p(stream.cuda_stream) if stream is not None else None,
                                            int(window_us), _ptr(out2), ctypes.byref(khz)))
        return khz.value

    def last_plan(self):
        """Geometry of the last decode_topk / score_topk* / mix_topk_exact on this thread (dae_last_plan).  n_tiles: the 32-column
        tiles the call WALKED -- those with a ranked column, ceil((min(n_tracks, col_hi) - col_lo) / 32), not the image's; a
        fused fp32 call splits them into n_sample_tiles + n_filter_tiles, a bf16 filter launch walks all of them again."""
        arr = (ctypes.c_int32 * 8)()
        self.lib.dae_last_plan(arr)
        keys = ["R_TILE", "n_rg", "nb_rg", "S", "n_sample_tiles", "n_filter_tiles", "fused",
                "n_tiles"]
        return dict(zip(keys, list(arr)))


class Catalogue:
    """Owns one dae_catalogue: an ascending list of global track columns and its inverse table on the device of `ctx`
    (dae_catalogue_create validates the list on the device: unsorted, repeated or non-track ids raise DaeError naming the first
    offender).  columns: an int32 CUDA tensor [n] (copied by the library).  Any context of that device ranks with it."""

    def __init__(self, ctx, columns, n_tracks):
        import torch
        self.ctx, self.h = ctx, None
        assert columns.dtype == torch.int32 and columns.is_cuda and columns.dim() == 1 and columns.is_contiguous()
        self.n, self.n_tracks = int(columns.numel()), int(n_tracks)
        h = ctypes.c_void_p()
        ctx.check(ctx.lib.dae_catalogue_create(ctx.h, _ptr(columns), self.n, self.n_tracks, ctypes.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.ctx.lib.dae_catalogue_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Block:
    """One polled feed's claim on a pinned result block of a Pipeline: released when the last array viewing it dies."""

    def __init__(self, pipe, block):
        self.pipe, self.block = pipe, block
        pipe._held[block] = pipe._held.get(block, 0) + 1

    def __del__(self):
        try:
            p = self.pipe
            n = p._held.get(self.block, 0) - 1
            if n > 0:
                p._held[self.block] = n
            else:
                p._held.pop(self.block, None)
            if p.h:
                p.lib.dae_pipeline_release(p.h, self.block)
                if p._closing and not p._held:           # close() was asked for while this array was alive
                    p.close()
        except Exception:
            pass


_live_pipelines = None          # weak set of open pipelines: closed at interpreter exit, BEFORE the HIP runtime tears down


def _close_pipelines_at_exit():
    for p in list(_live_pipelines or ()):
        try:
            p._held = {}
            p.close()
        except Exception:
            pass


class Pipeline:
    """The drivers' loop inside the library (include/dae_hip.h dae_pipeline_*): host feeds in, host top-k lists out; a
    library-owned thread issues the launches on `lanes` contexts.  The weights are CUDA tensors the caller keeps alive.
    `submit` / `results` from one thread."""

    def __init__(self, W_enc, b_enc, W_dec, b_dec, n_tracks, dtype=DAE_DTYPE_F32, k=500, group_rows=1024, max_nnz=1 << 20,
                 lanes=2, want_scores=True, result_blocks=None, device_index=0, title=None):
        """title: a models.title_models.Char_CNN with its variables on the device -> a titled pipeline
        (dae_pipeline_create_titled): `submit(..., titles=, titles_use=)` ranks the title-mixed score."""
        self.lib = load()
        V, H = W_enc.shape
        self._keep = (W_enc, b_enc, W_dec, b_dec, title)
        self.title_len = None if title is None else int(title.input_len)
        self.k, self.want_scores, self.group_rows, self.max_nnz = int(k), bool(want_scores), int(group_rows), int(max_nnz)
        h = ctypes.c_void_p()
        n_slots = 2 * lanes + 2              # launches the pipeline holds at once (csrc/pipeline.hip)
        n_blocks = max(int(result_blocks or 0), n_slots + 6)
        self._held = {}                      # result block -> claims of arrays still alive in the caller's hands
        self._closing = False
        self.max_held = n_blocks - n_slots                    # more blocks out than this: poll() copies instead of lending
        if title is None:
            rc = self.lib.dae_pipeline_create(int(device_index), _ptr(W_enc), _ptr(b_enc), _ptr(W_dec), _ptr(b_dec), V, H, int(n_tracks),
                                              int(dtype), int(k), int(group_rows), int(max_nnz), int(lanes), 1 if want_scores else 0,
                                              n_blocks, ctypes.byref(h))
        else:
            tm = title
            rc = self.lib.dae_pipeline_create_titled(
                int(device_index), _ptr(W_enc), _ptr(b_enc), _ptr(W_dec), _ptr(b_dec), V, H, int(n_tracks),
                _ptr(tm.p["char_embedding"]), tm.char_size, tm.embedding, _ptr(tm.p["conv_w"]), _ptr(tm.p["conv_b"]), tm._fs,
                len(tm.filter_sizes), tm.filter_num, _ptr(tm.p["Output_WT"]), _ptr(tm.p["Output_b"]), tm.ld, tm.input_len,
                int(dtype), int(k), int(group_rows), int(max_nnz), int(lanes), 1 if want_scores else 0, n_blocks, ctypes.byref(h))
        if rc != 0:
            raise DaeError("dae_pipeline_create failed (%d): %s" % (rc, self.lib.dae_pipeline_last_error(None).decode()))
        self.h = h
        self.eval = False
        self.cand = self.cand_rank = False
        self.pending = 0                     # feeds submitted and not yet yielded
        self.users = 0                       # streamed loops running on this pipeline (models/stream_loop.py)
        # the foreign calls' out-parameters, made once (a feed is ~25 us of this thread: five ctypes objects and their byref()
        # per poll were 3 us of it)
        self._t, self._n, self._b = ctypes.c_uint64(), ctypes.c_int(), ctypes.c_int()
        self._ip, self._sp = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_float)()
        self._poll_args = (ctypes.byref(self._t), ctypes.byref(self._ip), ctypes.byref(self._sp) if self.want_scores else None,
                           ctypes.byref(self._n), ctypes.byref(self._b))
        self._t_ref = ctypes.byref(self._t)
        self._rp = ctypes.c_void_p()
        self._poll_eval_args = (ctypes.byref(self._t), ctypes.byref(self._rp), ctypes.byref(self._n), ctypes.byref(self._b))
        # a pipeline owns a library thread and streams: it must be gone before the runtime is (a destructor running HIP calls
        # during interpreter teardown is undefined -- ADVICE r4)
        global _live_pipelines
        if _live_pipelines is None:
            import atexit
            import weakref
            _live_pipelines = weakref.WeakSet()
            atexit.register(_close_pipelines_at_exit)
        _live_pipelines.add(self)

    def _check(self, rc):
        if rc < 0:
            raise DaeError("dae_pipeline error %d: %s" % (rc, self.lib.dae_pipeline_last_error(self.h).decode()))
        return rc

    def enable_eval(self, max_answers=1 << 20):
        """The evaluation mode (dae_pipeline_enable_eval), before the first submit: every `submit` then carries `answers=`, and
        `poll_eval` hands out the rows' metric records instead of their lists.  The discount table is Python's own
        1 / math.log(p + 1, 2)."""
        from .utils.metrics import discount_table
        disc = discount_table(self.k)
        self._check(self.lib.dae_pipeline_enable_eval(self.h, disc.ctypes.data_as(ctypes.c_void_p), int(max_answers)))
        self.eval, self.max_answers = True, int(max_answers)

    def set_catalogue(self, cat):
        """Catalogue mode (dae_pipeline_set_catalogue), before the first submit: every launch ranks the columns of `cat` (a
        `Catalogue` of this device and of the pipeline's n_tracks); lists and metric records keep global columns.  The pipeline
        holds `cat` and so keeps it alive; close the pipeline before the catalogue."""
        self._check(self.lib.dae_pipeline_set_catalogue(self.h, cat.h))
        self._cat = cat

    def _feed_arrays(self, positions, values):
        import numpy as np
        if self._closing:
            raise DaeError("dae_pipeline: closed")
        pos = positions if (type(positions) is np.ndarray and positions.dtype == np.int64 and positions.flags.c_contiguous) \
            else np.ascontiguousarray(positions, np.int64)
        val = values if (type(values) is np.ndarray and values.dtype == np.float32 and values.flags.c_contiguous) \
            else np.ascontiguousarray(values, np.float32)
        nnz = pos.size >> 1
        if val.size != nnz and val.size != 1:
            raise ValueError("positions (%d) and values (%d) differ in length" % (nnz, val.size))
        return pos, val, nnz

    def submit(self, positions, values, n_rows, titles=None, titles_use=None, answers=None):
        """positions: int64 [nnz, 2] (C-contiguous numpy), values: float32 [nnz] or one value.  -> True, or False when every
        lane holds lists that were not fetched yet (take `results()` first).  titles [n_rows, L] int32 + titles_use [n_rows]
        (a titled pipeline): the launch ranks the title-mixed score.  answers=: `submit_eval` (a pipeline in evaluation mode,
        and only there)."""
        import numpy as np
        if answers is not None:
            return self.submit_eval(positions, values, n_rows, answers, titles, titles_use)
        pos, val, nnz = self._feed_arrays(positions, values)
        if titles is not None:
            tt = np.ascontiguousarray(titles, np.int32).reshape(-1)
            uu = np.ascontiguousarray(titles_use, np.float32).reshape(-1)
            if tt.size != int(n_rows) * self.title_len or uu.size != int(n_rows):
                raise ValueError("titles must be [n_rows, %d] and titles_use [n_rows]" % self.title_len)
            rc = self._check(self.lib.dae_pipeline_submit_titled(
                self.h, pos.ctypes.data_as(ctypes.c_void_p), val.ctypes.data_as(ctypes.c_void_p),
                1 if (val.size == 1 and nnz != 1) else 0, nnz, int(n_rows), tt.ctypes.data_as(ctypes.c_void_p),
                uu.ctypes.data_as(ctypes.c_void_p), self._t_ref))
        else:
            rc = self.lib.dae_pipeline_submit(self.h, ctypes.c_void_p(pos.__array_interface__["data"][0]),
                                              ctypes.c_void_p(val.__array_interface__["data"][0]),
                                              1 if (val.size == 1 and nnz != 1) else 0, nnz, int(n_rows), self._t_ref)
            if rc < 0:
                self._check(rc)
        if rc == DAE_PIPE_BUSY:
            return False
        self.pending += 1
        return True

    def submit_eval(self, positions, values, n_rows, answers, titles=None, titles_use=None):
        """`submit` on a pipeline in evaluation mode (`enable_eval`): the feed with its answers = (row_ptr int32 [n_rows + 1],
        col int32), a CSR over the feed's rows (-1 and duplicates allowed); `poll_eval` hands the rows' records out."""
        import numpy as np
        pos, val, nnz = self._feed_arrays(positions, values)
        arp = np.ascontiguousarray(answers[0], np.int32)
        acol = np.ascontiguousarray(answers[1], np.int32)
        if arp.size != int(n_rows) + 1 or arp[-1] > acol.size or arp[0] < 0:
            raise ValueError("answers: (row_ptr [n_rows + 1], col) with row_ptr[-1] <= len(col)")
        tt = uu = None
        if titles is not None:
            tt = np.ascontiguousarray(titles, np.int32).reshape(-1)
            uu = np.ascontiguousarray(titles_use, np.float32).reshape(-1)
            if tt.size != int(n_rows) * (self.title_len or 0) or uu.size != int(n_rows):
                raise ValueError("titles must be [n_rows, %s] and titles_use [n_rows]" % self.title_len)
        vp_ = ctypes.c_void_p
        rc = self._check(self.lib.dae_pipeline_submit_eval(
            self.h, pos.ctypes.data_as(vp_), val.ctypes.data_as(vp_), 1 if (val.size == 1 and nnz != 1) else 0, nnz, int(n_rows),
            None if tt is None else tt.ctypes.data_as(vp_), None if uu is None else uu.ctypes.data_as(vp_),
            arp.ctypes.data_as(vp_), acol.ctypes.data_as(vp_), self._t_ref))
        if rc == DAE_PIPE_BUSY:
            return False
        self.pending += 1
        return True

    def enable_candidates(self, max_candidates=1 << 20, rank=False, out_kind=DAE_OUT_SCORE):
        """The candidates mode (dae_pipeline_enable_candidates), before the first submit: every feed then goes through
        `submit_candidates`; `poll_candidates` hands out the listed pairs' values (rank=False), `poll` each row's k best
        candidates (rank=True)."""
        self._check(self.lib.dae_pipeline_enable_candidates(self.h, int(max_candidates), 1 if rank else 0, int(out_kind)))
        self.cand, self.cand_rank, self.max_candidates = True, bool(rank), int(max_candidates)
        self._cp, self._cn = ctypes.POINTER(ctypes.c_float)(), ctypes.c_int64()
        self._poll_cand_args = (ctypes.byref(self._t), ctypes.byref(self._cp), ctypes.byref(self._cn), ctypes.byref(self._n),
                                ctypes.byref(self._b))

    def submit_candidates(self, positions, values, n_rows, candidates, titles=None, titles_use=None):
        """`submit` on a pipeline in candidates mode: the feed with its candidates = (row_ptr int32 [n_rows + 1], col int32), a
        host CSR over the feed's rows (global column ids; -1 and duplicates allowed).  -> True, or False when every launch slot
        is taken (poll first)."""
        import numpy as np
        pos, val, nnz = self._feed_arrays(positions, values)
        crp, ccol = candidates
        if not (type(crp) is np.ndarray and crp.dtype == np.int32 and crp.flags.c_contiguous):
            crp = np.ascontiguousarray(crp, np.int32)
        if not (type(ccol) is np.ndarray and ccol.dtype == np.int32 and ccol.flags.c_contiguous):
            ccol = np.ascontiguousarray(ccol, np.int32)
        if crp.size != int(n_rows) + 1 or crp[-1] > ccol.size or crp[0] < 0:
            raise ValueError("candidates: (row_ptr [n_rows + 1], col) with row_ptr[-1] <= len(col)")
        tt = uu = None
        if titles is not None:
            tt = np.ascontiguousarray(titles, np.int32).reshape(-1)
            uu = np.ascontiguousarray(titles_use, np.float32).reshape(-1)
            if tt.size != int(n_rows) * (self.title_len or 0) or uu.size != int(n_rows):
                raise ValueError("titles must be [n_rows, %s] and titles_use [n_rows]" % self.title_len)
        vp_ = ctypes.c_void_p
        rc = self._check(self.lib.dae_pipeline_submit_candidates(
            self.h, vp_(pos.__array_interface__["data"][0]), vp_(val.__array_interface__["data"][0]),
            1 if (val.size == 1 and nnz != 1) else 0, nnz, int(n_rows),
            None if tt is None else tt.ctypes.data_as(vp_), None if uu is None else uu.ctypes.data_as(vp_),
            vp_(crp.__array_interface__["data"][0]), vp_(ccol.__array_interface__["data"][0]), self._t_ref))
        if rc == DAE_PIPE_BUSY:
            return False
        self.pending += 1
        return True

    def poll_candidates(self, wait=True, copy=False):
        """The next feed in submission order of a scoring candidates pipeline -> (values float32 [n_out] in the order of the
        feed's candidate ids, a view of the pinned result block as `poll` hands its lists out; bad: the feed's launch held an
        id outside -1 / [0, V), whose value is a NaN), or None when it is not ready (wait=False) or nothing is pending."""
        import numpy as np
        if self.pending == 0:
            return None
        rc = self.lib.dae_pipeline_poll_candidates(self.h, 1 if wait else 0, *self._poll_cand_args)
        if rc < 0:
            self._check(rc)
        if rc == DAE_PIPE_BUSY:
            raise DaeError("dae_pipeline: every result block is held (drop or copy the arrays of earlier feeds)")
        if self._n.value == 0:
            return None
        self.pending -= 1
        n, b = int(self._cn.value), self._b.value
        if n == 0:
            self._check(self.lib.dae_pipeline_release(self.h, b))
            return np.zeros(0, np.float32), rc == DAE_PIPE_BAD_ID
        copy = copy or (b not in self._held and len(self._held) >= self.max_held)
        owner = _Block(self, b)                  # (the block returns to the pipeline when the last array viewing it dies: `poll`)
        buf = (ctypes.c_float * n).from_address(ctypes.addressof(self._cp.contents))
        buf._owner = owner
        values = np.frombuffer(buf, dtype=np.float32)
        return (values.copy() if copy else values), rc == DAE_PIPE_BAD_ID

    def flush(self):
        self._check(self.lib.dae_pipeline_flush(self.h))

    def poll(self, wait=True, copy=False):
        """The next feed in submission order -> (idx [n_rows, k] int32, score or None), or None when it is not ready
        (wait=False) or nothing is pending.  The arrays VIEW a pinned result block that returns to the pipeline when they
        are garbage collected (copy=True: private copies, the block returns at once)."""
        import numpy as np
        if self.pending == 0:
            return None
        n, b, ip_, sp_ = self._n, self._b, self._ip, self._sp
        rc = self.lib.dae_pipeline_poll(self.h, 1 if wait else 0, *self._poll_args)
        if rc < 0:
            self._check(rc)
        if rc == DAE_PIPE_BUSY:
            raise DaeError("dae_pipeline: every result block is held (drop or copy the arrays of earlier feeds)")
        if n.value == 0:
            return None
        self.pending -= 1
        if b.value not in self._held and len(self._held) >= self.max_held:
            copy = True                      # the caller keeps many results alive: this one is copied, its block goes back
        owner = _Block(self, b.value)
        n_el = n.value * self.k

        def view(ptr, ctype, dt):
            # the ctypes array object is the memory owner numpy sees: it carries the block's claim, so every array derived
            # from the result (slices, views) keeps the block out of the pipeline's hands
            buf = (ctype * n_el).from_address(ctypes.addressof(ptr.contents))
            buf._owner = owner
            return np.frombuffer(buf, dtype=dt).reshape(n.value, self.k)
        idx = view(ip_, ctypes.c_int32, np.int32)
        score = view(sp_, ctypes.c_float, np.float32) if self.want_scores else None
        if copy:
            idx, score = idx.copy(), (None if score is None else score.copy())
        return idx, score

    def poll_eval(self, wait=True):
        """The next feed in submission order -> its rows' records (a numpy array of utils/metrics.py RECORD_DTYPE, a private
        copy: 24 bytes a row), or None when it is not ready (wait=False) or nothing is pending."""
        import numpy as np
        from .utils.metrics import RECORD_DTYPE
        if self.pending == 0:
            return None
        rc = self.lib.dae_pipeline_poll_eval(self.h, 1 if wait else 0, *self._poll_eval_args)
        if rc < 0:
            self._check(rc)
        n = self._n.value
        if n == 0:
            return None
        self.pending -= 1
        rec = np.frombuffer((ctypes.c_char * (n * RECORD_DTYPE.itemsize)).from_address(self._rp.value), dtype=RECORD_DTYPE).copy()
        self._check(self.lib.dae_pipeline_release(self.h, self._b.value))
        return rec

    def exact_margin(self, scale):
        self._check(self.lib.dae_pipeline_exact_margin(self.h, float(scale)))

    def times(self):
        """ms since creation: the library thread issuing / idle, the caller in submit / waiting in poll."""
        a = (ctypes.c_uint64 * 4)()
        self._check(self.lib.dae_pipeline_times(self.h, a))
        return dict(zip(("issue_ms", "idle_ms", "submit_ms", "wait_ms"), [round(int(x) / 1e6, 2) for x in a]))

    def stats(self):
        a = (ctypes.c_uint64 * 3)()
        self._check(self.lib.dae_pipeline_stats(self.h, a))
        return {"launches": int(a[0]), "feeds": int(a[1]), "guard_fallbacks": int(a[2])}

    def close(self):
        """Destroys the pipeline -- once no array handed out by poll() views its pinned blocks any more (until then the
        pipeline only stops taking feeds)."""
        if getattr(self, "h", None):
            if self._held:
                self._closing = True
                return
            self.lib.dae_pipeline_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self._held = {}              # (nothing can view the blocks any more: the claims hold a reference to this object)
            self.close()
        except Exception:
            pass
