"""MI355X-native backend for the batched augmented-ODE right-hand side of
ContinuousNormalizingFlows.jl (log-density evaluation): hand-written HIP kernels behind a C
ABI (``libcnfhip.so``, ``include/cnfhip.h``) plus this thin host mirror of the reference's
``construct`` / ``inference`` / ``loss`` / ``augmented_f`` / ``ICNFDist`` surface."""
import os as _os

# Kernel arguments in device memory instead of host memory: every step kernel starts by reading its
# argument block, and with the block behind PCIe that read costs ~2.5 us per launch (measured: 56.6 ->
# 54.0 us per fused step).  The HIP runtime reads the switch when it initialises, so it has to be in the
# environment before the first HIP call of the process; a value the user set is left alone.
# SIDE EFFECT, process-wide: importing this package sets HIP_FORCE_DEV_KERNARG=1 for every HIP user of the process, and
# it has NO effect if HIP was initialised before the import (e.g. `torch.cuda.init()` ran first): the library still works,
# each step launch just reads its arguments over PCIe.  `kernarg_in_device_memory()` tells which case holds.
_KERNARG_SET_HERE = "HIP_FORCE_DEV_KERNARG" not in _os.environ
_os.environ.setdefault("HIP_FORCE_DEV_KERNARG", "1")


def kernarg_in_device_memory():
    """True / False when it is known whether the HIP runtime saw HIP_FORCE_DEV_KERNARG=1 at initialisation, None when
    the variable was set by this import but torch had already initialised HIP (so the runtime never read it)."""
    if _os.environ.get("HIP_FORCE_DEV_KERNARG") != "1":
        return False
    if not _KERNARG_SET_HERE:
        return True
    try:
        import torch
        return None if (torch.cuda.is_initialized() and not _HIP_COLD_AT_IMPORT) else True
    except ImportError:
        return True


def _hip_cold():
    import sys as _sys
    t = _sys.modules.get("torch")
    try:
        return t is None or not t.cuda.is_initialized()
    except Exception:
        return True


_HIP_COLD_AT_IMPORT = _hip_cold()

from . import _lib
from ._lib import CNFError, build
from .base_icnf import (ICNF, ODEProblem, base_sol, construct, generate, generate_prob, generate_sol,
                        inference, inference_collect, inference_prob, inference_submit,
                        inference_sol, loss, loss_and_grad, loss_and_grad_collect, loss_and_grad_submit, loss_from_sums, loss_sums, n_augment,
                        n_augment_input, steer_tspan)
from .base_icnf import base_logpdf_pullback, base_sample, base_sample_pullback
from .dist import CondICNFDist, ICNFDist, ICNFDistribution, logpdf, pdf, rand, rand_
from . import distributions
from .distributions import DiagNormal, LearnableNormal, MvNormal, Rademacher, StdNormal
from .icnf import augmented_f
from .layers import Chain, CondLayer, Dense, PlanarLayer, setup
from . import rng
from .rng import HIPRNG
from .types import (FFJORD, RNODE, CondFFJORD, CondPlanar, CondRNODE, HIPJacVecMatrixMode,
                    HIPMatrixMode, HIPVecJacMatrixMode, Planar, TestMode, TrainMode)
from .vjp import differentiable_inference, inference_pullback, inference_record, tempered_loss, weighted_loss
from .gen_vjp import differentiable_generate, generate_pullback, generate_record, reverse_kl
from . import ensemble, gen_vjp, mlj, parallel, vjp
from .ensemble import ensemble_capacity, ensemble_steps, fit_many, loss_and_grad_many
from .ensemble import EnsembleDist, ensemble_eval_capacity, ensemble_eval_steps, generate_many, inference_many, logpdf_members, \
    loss_many
from .ensemble import differentiable_inference_many, ensemble_vjp_capacity, inference_vjp_many
from .ensemble import differentiable_generate_many, ensemble_generate_vjp_capacity, generate_vjp_many, reverse_kl_many
from .ensemble import member_loss_from_sums, member_twin, pad_columns      # heterogeneous members: counts, lambdas, tolerances
from . import ensemble_base
from .ensemble_base import EnsembleBases                                   # a base distribution per member: bases=
from . import path
from .path import generate_path, inference_path, solve_path
from . import path_vjp
from .path_vjp import differentiable_generate_path, differentiable_inference_path, generate_path_vjp, inference_path_vjp, \
    path_vjp_max_batch, path_vjp_steps
from . import ensemble_path
from .ensemble_path import differentiable_generate_path_many, differentiable_inference_path_many, ensemble_path_capacity, \
    ensemble_path_steps, ensemble_path_vjp_capacity, generate_path_many, generate_path_vjp_many, inference_path_many, \
    inference_path_vjp_many
from . import jvp
from .jvp import generate_jvp, inference_jvp, jvp_steps, loss_jvp
from . import ensemble_jvp
from .ensemble_jvp import ensemble_jvp_steps, generate_jvp_many, inference_jvp_many, loss_jvp_many, loss_jvp_reduce
from .mlj import (Adam, CondICNFModel, ICNFModel, Lion, Machine, fit, fit_, fitted_params, load_params, machine, save_params,
                  transform)

__all__ = [n for n in dir() if not n.startswith("_")]
