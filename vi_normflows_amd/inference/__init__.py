"""Estimators, schedules, optimizers and training drivers."""
from .annealing import get_schedule, reference_schedule, theano_schedule
from .bbvi import black_box_vi, black_box_vi_full_rank, linreg_log_joint, linreg_posterior
from .elbo import FreeEnergy, amortized_free_energy, free_energy, reference_free_energy
from .flow_vi import FlowVI, fit_density, fit_flow_vi, optimise
from .hmc import HMC, HMCResult, ess, fit_hmc, moment_gap, split_rhat
from .laplace import LaplaceResult, fit_laplace, laplace, newton_map
from .optimizers import make_optimizer
from .svgd import SVGD, SVGDResult, fit_svgd, flow_ksd, score_fn
from .trainer import TrainConfig, Trainer

__all__ = ["get_schedule", "reference_schedule", "theano_schedule", "black_box_vi",
           "black_box_vi_full_rank",
           "linreg_log_joint", "linreg_posterior", "FreeEnergy", "free_energy",
           "reference_free_energy", "amortized_free_energy", "FlowVI", "fit_flow_vi", "fit_density", "optimise",
           "make_optimizer", "TrainConfig", "Trainer", "SVGD", "SVGDResult", "fit_svgd", "flow_ksd",
           "score_fn", "HMC", "HMCResult", "fit_hmc", "split_rhat", "ess", "moment_gap",
           "LaplaceResult", "fit_laplace", "laplace", "newton_map"]
