"""
vidp_amd -- MI355X-native block-tri-diagonal Gauss-Markov path for the VDP / CVI-DP ELBO.

Only the hot path of AaltoML/vi-diffusion-processes behind the reference's own
interface names; compute happens in hand-written HIP kernels (csrc/) reached through a C ABI.
"""
from . import _lib  # noqa: F401
from .packed import Plan  # noqa: F401
from ._lib import FULL, SYM, TRI, VEC  # noqa: F401


def __getattr__(name):
    # the models import the kernels and the plan machinery: loaded on first use
    if name == "SpatioTemporalSparseCVI":
        from .spatio_temporal_variational import SpatioTemporalSparseCVI
        return SpatioTemporalSparseCVI
    if name == "MultiLatentSparseCVI":
        from .multi_latent_variational import MultiLatentSparseCVI
        return MultiLatentSparseCVI
    if name == "PanelSparseCVI":
        from .panel_variational_cvi import PanelSparseCVI
        return PanelSparseCVI
    if name in ("MeanFunction", "ZeroMeanFunction", "LinearMeanFunction", "ImpulseMeanFunction", "StepMeanFunction"):
        from . import mean_function
        return getattr(mean_function, name)
    if name == "FactorAnalysisSparseCVI":
        from .factor_analysis_variational import FactorAnalysisSparseCVI
        return FactorAnalysisSparseCVI
    if name == "MiniBatchSitesTrainer":
        from .trainers import MiniBatchSitesTrainer
        return MiniBatchSitesTrainer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
