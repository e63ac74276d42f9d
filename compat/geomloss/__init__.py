"""Opt-in stand-in for the third-party ``geomloss`` package: its ``SamplesLoss`` for the debiased Sinkhorn divergence
(p = 2) on this project's HIP kernels.  Not on the default path: put this directory in front of the repository on
PYTHONPATH (``PYTHONPATH=<repo>/compat:<repo>``) to have ``from geomloss import SamplesLoss`` pick it up."""
from diffsound_amd.ddsp.sinkhorn import SamplesLoss

__all__ = ["SamplesLoss"]
