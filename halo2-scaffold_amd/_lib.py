"""ctypes binding of libh2mi.so (include/h2mi.h).  Fails loudly when the library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))


def lib_path() -> str:
    """the product library next to this file; H2MI_LIBRARY=<path> selects another product build (tools/ab_lib.sh and
    tools/ab_host.sh compare two builds that way)"""
    return os.environ.get("H2MI_LIBRARY") or os.path.join(_HERE, "libh2mi.so")


class H2miError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = code
        msg = lib.h2mi_strerror(code).decode() if lib is not None else "?"
        super().__init__(f"h2mi error {code} ({msg}) {where}")


def _load():
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError(
            f"{p} not found: build it with `make -C halo2-scaffold_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback for the MSM/NTT path."
        )
    L = C.CDLL(p, mode=C.RTLD_GLOBAL)
    u64p = C.POINTER(C.c_uint64)
    vp = C.c_void_p
    sz = C.c_size_t
    sig = {
        "h2mi_init": ([C.c_int], C.c_int),
        "h2mi_init_devices": ([C.c_int], C.c_int),
        "h2mi_device_count": ([], C.c_int),
        "h2mi_primary_device": ([], C.c_int),
        "h2mi_shutdown": ([], None),
        "h2mi_strerror": ([C.c_int], C.c_char_p),
        "h2mi_version": ([], C.c_char_p),
        "h2mi_malloc": ([sz, C.POINTER(vp)], C.c_int),
        "h2mi_free": ([vp], C.c_int),
        "h2mi_memcpy_h2d": ([vp, vp, sz], C.c_int),
        "h2mi_memcpy_h2d_async": ([vp, vp, sz], C.c_int),
        "h2mi_memcpy_d2h": ([vp, vp, sz], C.c_int),
        "h2mi_fr_patch_cells_dev": ([vp, vp, sz, vp], C.c_int),
        "h2mi_memcpy_d2d": ([vp, vp, sz], C.c_int),
        "h2mi_memset_zero": ([vp, sz], C.c_int),
        "h2mi_sync": ([], C.c_int),
        "h2mi_join": ([], C.c_int),
        "h2mi_msm_flush": ([], C.c_int),
        "h2mi_bases_register": ([vp, sz, u64p], C.c_int),
        "h2mi_bases_register_dev": ([vp, sz, u64p], C.c_int),
        "h2mi_bases_register_depth": ([vp, sz, C.c_uint32, u64p], C.c_int),
        "h2mi_bases_register_depth_dev": ([vp, sz, C.c_uint32, u64p], C.c_int),
        "h2mi_bases_memory": ([C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64p, u64p], C.c_int),
        "h2mi_bases_release": ([C.c_uint64], C.c_int),
        "h2mi_bases_info": ([C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), u64p], C.c_int),
        "h2mi_msm_bn254_g1": ([C.c_uint64, vp, vp, sz, vp], C.c_int),
        "h2mi_msm_bn254_g1_dev": ([C.c_uint64, vp, sz, vp, vp], C.c_int),
        "h2mi_msm_bn254_g1_phase_dev": ([C.c_uint64, vp, sz, sz, vp, C.c_uint, vp], C.c_int),
        "h2mi_msm_adhoc_builds": ([u64p], C.c_int),
        "h2mi_msm_last_stats": ([C.c_uint64, u64p, u64p], C.c_int),
        "h2mi_msm_set_canonical": ([C.c_int], C.c_int),
        "h2mi_fe_to_repr_dev": ([C.c_int, vp, sz, vp, vp], C.c_int),
        "h2mi_fe_from_repr_dev": ([C.c_int, vp, sz, vp, u64p], C.c_int),
        "h2mi_g1_compress_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_g1_decompress_dev": ([vp, sz, vp, u64p], C.c_int),
        "h2mi_g1_compress": ([vp, sz, vp], C.c_int),
        "h2mi_g1_decompress": ([vp, sz, vp, u64p], C.c_int),
        "h2mi_g1_sum_jacobian": ([vp, sz, vp], C.c_int),
        "h2mi_g1_fold_groups": ([vp, sz, sz, vp], C.c_int),
        "h2mi_g1_batch_normalize": ([vp, sz, vp], C.c_int),
        "h2mi_g1_fold_groups_dev": ([vp, sz, sz, vp, vp], C.c_int),
        "h2mi_g1_batch_normalize_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_library_stream": ([C.POINTER(vp)], C.c_int),
        "h2mi_stream_create": ([C.POINTER(vp)], C.c_int),
        "h2mi_stream_destroy": ([vp], C.c_int),
        "h2mi_stream_wait": ([vp, vp], C.c_int),
        "h2mi_fr_add_head_dev": ([vp, vp, sz, vp], C.c_int),
        "h2mi_fr_fill_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_fr_mul_dev": ([vp, vp, sz, vp, vp], C.c_int),
        # assigned cells: ff's BatchInvert, Assigned::evaluate over a vector, and the rational cells of several columns in one chain
        "h2mi_fr_batch_invert_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_fr_assigned_evaluate_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_fr_assigned_columns_dev": ([vp, C.c_uint32, C.c_int, u64p, vp], C.c_int),
        # witness cells from device memory / as 64-bit integers: one k_cells_scatter launch for up to 64 columns
        "h2mi_fr_scatter_cells_dev": ([vp, C.c_uint32, u64p, vp], C.c_int),
        "h2mi_fr_scatter_cells_staged_dev": ([vp, C.c_uint32, C.c_uint64, u64p, vp], C.c_int),
        # the inverse: device columns -> their nonzero cells in row order (count, prefix, ordered scatter; no atomic)
        "h2mi_fr_compact_cells_dev": ([vp, C.c_uint32, C.c_uint, vp, vp, vp], C.c_int),
        # witness programs: a recorded builder closure evaluated on the device (csrc/h2mi_witness.hip)
        "h2mi_witness_check": ([vp], C.c_int),
        "h2mi_witness_create": ([vp, C.POINTER(vp)], C.c_int),
        "h2mi_witness_info": ([vp, vp], C.c_int),
        "h2mi_witness_run": ([vp, vp, vp, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_witness_read": ([vp, vp, C.c_uint32, vp], C.c_int),
        "h2mi_witness_release": ([vp], C.c_int),
        "h2mi_fr_random_dev": ([vp, sz, C.c_uint64, C.c_uint64, vp], C.c_int),
        "h2mi_fr_random_chacha_dev": ([vp, sz, vp, C.c_uint64, C.c_uint64, vp], C.c_int),
        "h2mi_ntt_bn254_fr": ([vp, vp, C.c_uint32], C.c_int),
        "h2mi_ntt_ext_bn254_fr": ([vp, C.c_uint32, vp, vp, vp], C.c_int),
        "h2mi_ntt_bn254_fr_dev": ([vp, C.c_uint32, vp, vp, vp, vp], C.c_int),
        "h2mi_ntt_bn254_fr_oop_dev": ([vp, sz, vp, C.c_uint32, vp, vp, vp, vp], C.c_int),
        "h2mi_fr_scale_powers_dev": ([vp, sz, vp, vp, vp], C.c_int),
        "h2mi_fr_eval_poly_dev": ([vp, sz, vp, vp, vp], C.c_int),
        "h2mi_fr_eval_polys_dev": ([vp, sz, sz, vp, vp, vp], C.c_int),
        "h2mi_fr_eval_polys_multi_dev": ([vp, vp, vp, sz, sz, vp, vp], C.c_int),
        "h2mi_fr_powtab_prefetch_dev": ([vp, sz, sz, vp], C.c_int),
        "h2mi_plonk_permutation_products_dev": ([vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_permutation_products_sparse_dev": ([vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.c_uint32, vp, vp],
                                                       C.c_int),
        "h2mi_fr_kate_division_dev": ([vp, sz, vp, vp, vp, vp], C.c_int),
        "h2mi_fr_kate_division_multi_dev": ([vp, sz, vp, vp, vp, sz, vp, vp], C.c_int),
        "h2mi_fr_lincomb_dev": ([vp, vp, sz, sz, vp, vp], C.c_int),
        "h2mi_fr_gwc_witness_dev": ([vp, vp, vp, vp, vp, sz, sz, vp, vp], C.c_int),
        # the quotient calls: (cosets or h2mi_quotient_circuits, h2mi_quotient_scalars, [slice,] out, stream); plonk.py mirrors the records
        "h2mi_plonk_evaluate_h_standard_dev": ([vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_evaluate_h_range_dev": ([vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_evaluate_h_flex_dev": ([vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_evaluate_h_expr_dev": ([vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_evaluate_h_expr_batch_dev": ([vp, vp, C.c_int32, vp, vp], C.c_int),
        # (h2mi_expr_columns, domain_k, theta, out, stream) / (h2mi_expr_columns, n_rows, report, n_polys, stream)
        "h2mi_plonk_expr_compress_dev": ([vp, C.c_uint32, vp, vp, vp], C.c_int),
        "h2mi_plonk_expr_check_dev": ([vp, C.c_uint32, vp, C.POINTER(C.c_uint32), vp], C.c_int),
        "h2mi_plonk_permutation_product_dev": ([vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_lookup_permute_dev": ([vp, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, u64p, vp], C.c_int),
        "h2mi_plonk_instance_coset_dev": ([vp, C.c_uint32, C.c_uint32, vp, sz, vp, vp], C.c_int),
        "h2mi_plonk_lookup_product_dev": ([vp, vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp, vp], C.c_int),
        "h2mi_plonk_shuffle_product_dev": ([vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp], C.c_int),
        "h2mi_plonk_logup_multiplicity_dev": ([vp, vp, C.c_uint32, C.c_uint32, vp, u64p, vp], C.c_int),
        "h2mi_plonk_logup_sum_dev": ([vp, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp], C.c_int),
        "h2mi_plonk_logup_multiplicity_sets_dev": ([vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, u64p, vp], C.c_int),
        "h2mi_plonk_logup_sum_sets_dev": ([vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, vp, vp], C.c_int),
        "h2mi_plonk_logup_rank_cols_dev": ([vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, vp, u64p, vp], C.c_int),
        "h2mi_plonk_logup_sum_ranked_dev": ([vp, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp, vp, vp], C.c_int),
        # several instance columns (h2mi_instance_cosets)
        "h2mi_plonk_instance_coset_multi_dev": ([vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp], C.c_int),
        "h2mi_plonk_copy_check_dev": ([vp, C.c_uint32, vp, C.c_uint32, vp, vp], C.c_int),
        "h2mi_plonk_lookup_member_dev": ([vp, vp, C.c_uint32, C.c_uint32, vp, vp], C.c_int),
        "h2mi_plonk_shuffle_member_dev": ([vp, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp, vp], C.c_int),
        "h2mi_fr_sort_unique_dev": ([vp, C.c_uint32, vp, vp, vp, C.POINTER(C.c_uint32), vp], C.c_int),
        "h2mi_fr_sort_unique_first_dev": ([vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(C.c_uint32), vp], C.c_int),
        "h2mi_g1_fixed_base_mul_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_fr_powers_dev": ([vp, sz, vp, vp], C.c_int),
        "h2mi_fft_bn254_g1_dev": ([vp, vp, C.c_uint32, vp, vp, vp], C.c_int),
        "h2mi_profile_enable": ([C.c_int], C.c_int),
        "h2mi_profile_filter": ([C.c_char_p], C.c_int),
        "h2mi_profile_reset": ([], C.c_int),
        "h2mi_profile_dump": ([C.c_char_p, sz, C.POINTER(sz)], C.c_int),
        "h2mi_profile_query": ([C.c_char_p, C.POINTER(C.c_double), u64p], C.c_int),
        # include/h2mi_prover.h: the resident prover behind its phase-level ABI
        "h2mi_prover_keygen": ([vp, C.POINTER(vp)], C.c_int),
        "h2mi_column_cells_check": ([vp, C.c_uint32, C.c_uint], C.c_int),
        "h2mi_gate_program_check": ([vp, vp, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_shape_gate_program": ([vp, vp, C.c_uint32, C.POINTER(C.c_uint32), vp, C.c_uint32, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_lookup_program_check": ([vp, vp, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_advice_phases_check": ([vp, vp, vp, vp], C.c_int),
        "h2mi_shuffle_program_check": ([vp, vp, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_shuffle_phases_check": ([vp, vp, vp, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_logup_inputs_check": ([vp, vp, vp, vp, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_table_logup_check": ([vp, vp, C.POINTER(C.c_uint32)], C.c_int),
        "h2mi_prover_pk_release": ([vp], C.c_int),
        # proving-key files: one self-describing blob out of HBM and back
        "h2mi_prover_pk_export": ([vp, vp, sz, vp, sz, C.POINTER(sz)], C.c_int),
        "h2mi_prover_pk_import": ([vp, sz, C.c_uint64, C.c_uint, C.POINTER(vp)], C.c_int),
        "h2mi_prover_pk_blob_check": ([vp, sz, vp, C.POINTER(vp), C.POINTER(sz)], C.c_int),
        "h2mi_prover_vk_commitments": ([vp, vp, vp], C.c_int),
        "h2mi_prover_create": ([vp, C.c_uint64, C.c_uint64, sz, sz, C.POINTER(vp)], C.c_int),
        "h2mi_prover_destroy": ([vp], C.c_int),
        "h2mi_prover_set_combiner": ([vp, vp, vp, vp, vp], C.c_int),
        "h2mi_prover_set_rng_key": ([vp, vp], C.c_int),
        "h2mi_prover_get_counts": ([vp, vp], C.c_int),
        "h2mi_prover_instances": ([vp, vp], C.c_int),
        "h2mi_prover_advice": ([vp, vp, vp, sz, C.c_uint64, vp], C.c_int),
        "h2mi_prover_advice_phase": ([vp, C.c_uint32, vp, vp, sz, C.c_uint64, vp], C.c_int),
        "h2mi_prover_set_challenges": ([vp, vp], C.c_int),
        "h2mi_prover_get_phase_counts": ([vp, vp], C.c_int),
        "h2mi_prover_check": ([vp, vp, vp, sz, C.POINTER(sz)], C.c_int),
        "h2mi_prover_lookups": ([vp, vp, vp], C.c_int),
        "h2mi_prover_products": ([vp, vp, vp, vp], C.c_int),
        "h2mi_prover_quotient": ([vp, vp, vp], C.c_int),
        "h2mi_prover_num_evaluations": ([vp, C.POINTER(sz)], C.c_int),
        "h2mi_prover_evaluations": ([vp, vp, vp], C.c_int),
        "h2mi_prover_shplonk_quotient": ([vp, vp, vp, vp], C.c_int),
        "h2mi_prover_shplonk_open": ([vp, vp, vp], C.c_int),
        "h2mi_prover_gwc_num_points": ([vp, vp], C.c_int),
        "h2mi_prover_gwc_open": ([vp, vp, vp], C.c_int),
        "h2mi_batch_create": ([vp, C.c_uint32, C.POINTER(vp)], C.c_int),
        "h2mi_batch_destroy": ([vp], C.c_int),
        "h2mi_batch_quotient": ([vp, vp, vp], C.c_int),
        "h2mi_batch_num_evaluations": ([vp, C.POINTER(sz)], C.c_int),
        "h2mi_batch_evaluations": ([vp, vp, vp], C.c_int),
        "h2mi_batch_shplonk_quotient": ([vp, vp, vp, vp], C.c_int),
        "h2mi_batch_shplonk_open": ([vp, vp, vp], C.c_int),
        "h2mi_batch_gwc_num_points": ([vp, vp], C.c_int),
        "h2mi_batch_gwc_open": ([vp, vp, vp], C.c_int),
        "h2mi_prover_buffer": ([vp, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(sz)], C.c_int),
        "h2mi_prover_pk_buffer": ([vp, C.c_uint32, C.c_uint32, C.POINTER(vp), C.POINTER(sz)], C.c_int),
        "h2mi_prover_device_bytes": ([vp, C.POINTER(sz), C.POINTER(sz)], C.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)  # AttributeError here = a symbol the header declares is missing
        fn.argtypes = args
        fn.restype = res
    L._h2mi_symbols = tuple(sig)
    return L


lib = None
lib = _load()


def check(code, where=""):
    if code != 0:
        raise H2miError(code, where)


def init(device=None):
    """h2mi_init on LOCAL_RANK (one process per GPU) unless a device is given."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    check(lib.h2mi_init(int(device)), "h2mi_init")
    return device
