"""Normalizing-flow layers: planar, radial, diagonal affine, RealNVP coupling, MADE/IAF/MAF,
rational-quadratic spline (coupling and autoregressive), Sylvester, neural autoregressive (deep
sigmoidal), LU-parameterised linear and triangular affine."""
from .affine import DiagAffine
from .base import Flow, FlowDistribution, FlowSequence, Permute, Reverse
from .coupling import AffineCoupling, RealNVP, coupling_transform
from .linear import LULinear, TriangularAffine
from .made import IAF, MADE, MAF, MaskedLinear, made_degrees, made_masks
from .naf import DSFAutoregressive, DSFCoupling, NeuralAutoregressiveFlow
from .planar import (AmortizedPlanar, Planar, PlanarStack, get_uhat, m, planar_flow,
                     planar_stack, planar_stack_inverse, planar_stack_inverse_reference,
                     planar_stack_reference)
from .radial import (AmortizedRadial, Radial, RadialStack, radial_params, radial_stack,
                     radial_stack_inverse, radial_stack_inverse_reference,
                     radial_stack_reference)
from .spline import MaskedSplineFlow, NeuralSplineFlow, RQSAutoregressive, RQSCoupling
from .sylvester import AmortizedSylvester, SylvesterStack

__all__ = [
    "Flow", "FlowSequence", "FlowDistribution", "Permute", "Reverse", "DiagAffine",
    "AffineCoupling", "RealNVP", "coupling_transform", "MADE", "IAF", "MAF", "MaskedLinear",
    "made_degrees", "made_masks", "Planar", "PlanarStack", "AmortizedPlanar", "get_uhat", "m",
    "planar_flow", "planar_stack", "planar_stack_reference", "Radial", "RadialStack",
    "AmortizedRadial", "radial_params", "radial_stack", "radial_stack_reference",
    "RQSCoupling", "NeuralSplineFlow", "RQSAutoregressive", "MaskedSplineFlow",
    "SylvesterStack", "AmortizedSylvester",
    "DSFCoupling", "DSFAutoregressive", "NeuralAutoregressiveFlow",
    "planar_stack_inverse", "planar_stack_inverse_reference", "radial_stack_inverse",
    "radial_stack_inverse_reference", "LULinear", "TriangularAffine",
]
