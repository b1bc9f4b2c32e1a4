"""nuts_rs_amd — MI355X-native many-chain NUTS engine behind the nuts-rs chain-driver interface.

The compute path is hand-written HIP for gfx950 in csrc/ exposed through the C ABI of include/nuts_amd.h
(libnuts_amd.so); this package is the thin host-side mirror of the reference's Settings/Chain interface.
Importing the package does not need a GPU; creating a ChainBatch does (there is no CPU fallback).
"""
from ._lib import NM_QUANTILE_MAX_PROBS, NM_RANK_SLAB_KEYS, NM_TRANSFORM_FOLDED_RANK_NORMAL, NM_TRANSFORM_INDICATOR_LE, NM_TRANSFORM_RANK_NORMAL, NM_SCATTER_MAX_DIM, NM_SCATTER_MAX_SLABS, NM_SCATTER_SLAB_MIN_ROWS, NM_SUMMARY_CHUNK_CHAINS, NutsAmdError, STATS_DTYPE, VECTOR_STATS, load as load_library  # noqa: F401
from .sampler import (AdamOptions, ChainBatch, DiagAdaptExpSettings, DiagNutsSettings, DualAverageOptions,  # noqa: F401
                      EuclideanAdaptOptions, LogpSpec, LowRankNutsSettings, KineticEnergyKind, DiagMclmcSettings, LowRankMclmcSettings, MclmcTrajectoryKind, RecoverableLogpError, LowRankSettings, Progress, StepSizeSettings, RankDiagnostics, RankSummary, Summary, quantile_draws, rank_diagnostics, sample, summarize_draws, transform_draws,
                      ADAPT_DIAG, ADAPT_LOW_RANK,
                      LOGP_IID_NORMAL, LOGP_DIAG_NORMAL, LOGP_FUNNEL, LOGP_EIGHT_SCHOOLS, LOGP_MVN_PREC, LOGP_MODULE, LOGP_HOST_CALLBACK,
                      STEP_DUAL_AVERAGE, STEP_ADAM, STEP_FIXED)

from ._lib import NM_DIAG_ALL, NM_DIAG_SAMPLING, NM_DIAG_TUNING, NM_DIAG_DEPTH_BINS, NM_STAT_WORDS  # noqa: F401
from .sampler import SamplerDiagnostics, sampler_diagnostics, stats_columns  # noqa: F401
from .pooled import covariance_draws, pooled_scatter  # noqa: F401
from .controller import ChainProgress, ProgressCallback, Sampler, SamplerWaitResult  # noqa: F401

__all__ = ["ChainProgress", "ProgressCallback", "Sampler", "SamplerWaitResult", "AdamOptions", "ChainBatch", "DiagNutsSettings", "EuclideanAdaptOptions", "StepSizeSettings", "DualAverageOptions",
           "DiagAdaptExpSettings", "LowRankNutsSettings", "KineticEnergyKind", "DiagMclmcSettings", "LowRankMclmcSettings", "MclmcTrajectoryKind", "LowRankSettings", "LogpSpec", "Progress", "sample", "NutsAmdError", "STATS_DTYPE", "VECTOR_STATS",
           "load_library", "Summary", "summarize_draws", "NM_SUMMARY_CHUNK_CHAINS", "quantile_draws", "NM_QUANTILE_MAX_PROBS",
           "transform_draws", "rank_diagnostics", "RankDiagnostics", "RankSummary", "NM_RANK_SLAB_KEYS", "NM_TRANSFORM_RANK_NORMAL", "NM_TRANSFORM_FOLDED_RANK_NORMAL", "NM_TRANSFORM_INDICATOR_LE",
           "covariance_draws", "pooled_scatter", "NM_SCATTER_SLAB_MIN_ROWS", "NM_SCATTER_MAX_SLABS", "NM_SCATTER_MAX_DIM",
           "stats_columns", "sampler_diagnostics", "SamplerDiagnostics", "NM_STAT_WORDS", "NM_DIAG_ALL", "NM_DIAG_SAMPLING", "NM_DIAG_TUNING", "NM_DIAG_DEPTH_BINS"]
