"""MI355X-native Twisted-Edwards-BLS12 MSM engine: host-side mirror of the reference's entry point.

The product is `libtemsm.so` (hand-written HIP kernels for gfx950 + the C-ABI of include/te_msm.h).
This package is the thin Python host layer over that C-ABI used by tests, bench.py and
multi-process (one rank per GPU) deployments; the JavaScript host layer that keeps the reference's
`compute_msm(bufferPoints, bufferScalars)` signature lives in js/ (see INTEGRATION.md).

The directory name contains hyphens (it is the reference's name + `_amd`), so import it with
    importlib.import_module("webgpu-msm-twisted-edwards_amd")
There is no CPU fallback anywhere in this package: without libtemsm.so and a HIP device every entry
point raises.
"""
from .binding import (  # noqa: F401
    Base,
    Bases,
    MsmContext,
    MsmError,
    compute_msm,
    set_bases,
    finalize_host,
    host_tail_features,
    finalize_gathered,
    finalize_sum,
    devices_from_env,
    synth_inputs,
    build_library,
    library_path,
    PARTIAL_BYTES,
    PARTIAL_BYTES_BLS12_377,
    partial_bytes,
    CURVE_TE_BLS12,
    CURVE_BLS12_377_G1,
    WORKSETS,
    MAX_BATCH,
    BATCH_SEQ_MAX,
    EPOINT,
    POINT_NONCANONICAL,
    POINT_OFF_CURVE,
    POINT_NOT_IN_SUBGROUP,
    X_BYTES,
    X_BYTES_BLS12_377,
    EFIELD,
    FIELD_P,
    FIELD_Q377,
    FIELD_ADD,
    FIELD_SUB,
    FIELD_MUL,
    FIELD_DOUBLE,
    FIELD_NEG,
    FIELD_SQUARE,
    FIELD_INV,
    FIELD_POW,
    FIELD_SQRT,
    FIELD_SHARED_B,
    FIELD_MONTGOMERY,
    FIELD_ZERO_OK,
    FIELD_ZERO,
    FIELD_NOT_SQUARE,
    NTT_INVERSE,
    NTT_MONTGOMERY,
    NTT_MAX_LOG_N,
    POLY_MONTGOMERY,
    POLY_SHARED_Z,
    POLY_MAX_N,
    SCAN_SUM,
    SCAN_PRODUCT,
    SCAN_MONTGOMERY,
    SCAN_EXCLUSIVE,
    SCAN_SHARED_A,
    SCAN_MAX_N,
    MATRIX_MONTGOMERY,
    MATRIX_TRANSPOSE,
    SPMV_MONTGOMERY,
    SPMV_TRANSPOSE,
    Matrix,
)
from .sharding import ShardedPipeline, compute_msm_sharded, distribute_inputs, exchange_partials, merge_partials, rows_of_batched_msm, window_shard_for_rank  # noqa: F401
