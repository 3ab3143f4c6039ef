"""lagomorph_amd -- MI355X-native LDDMM hot path behind lagomorph's operator surface.

Importing this package requires the built HIP library (no CPU fallback).
"""
import sys as _sys

# `python -m lagomorph_amd.build` imports this package before it runs the builder; with no library yet
# that must not fail (everything else does: there is no CPU fallback).
_BUILDING = "lagomorph_amd.build" in getattr(_sys, "orig_argv", [])

if not _BUILDING:
    from .adjrep import *  # noqa: F401,F403
    from .adjrep import Ad, Ad_dagger, Ad_star, ad, ad_dagger, ad_star, sym, sym_dagger  # noqa: F401
    from .affine import (AffineInterp, AffineInterpFunction, RegridFunction, RegridModule, StandardizedDataset,  # noqa: F401
                         affine_atlas, affine_interp, batch_average, load_affine_atlas, save_affine_atlas,
                         affine_inverse, det_2x2, invert_2x2, invert_3x3, regrid, rigid_inverse, rotation_exp_map)
    from .bspline import (BsplinePrefilterFunction, InterpBsplineFunction, bspline_prefilter, interp_bspline,  # noqa: F401
                          interp_cubic)
    from .deform import (InterpFunction, InvertDisplacementFunction, compose, compose_disp_vel,  # noqa: F401
                         compose_vel_disp, identity, interp, interp_hessian_diagonal_image, invert_displacement)
    from .diff import (JacobianDeterminantFunction, JacobianTimesVectorFieldAdjointFunction,  # noqa: F401
                       JacobianTimesVectorFieldFunction, jacobian_determinant, jacobian_times_vectorfield,
                       jacobian_times_vectorfield_adjoint)
    from .distance import distance_transform, signed_distance, surface_distance, surface_mask  # noqa: F401
    from .ffd import FFDFunction, ffd_expand, ffd_grid_shape, ffd_restrict  # noqa: F401
    from .labels import dice, label_overlap, warp_labels  # noqa: F401
    from .lagomorph_ext import set_debug_mode  # noqa: F401
    from .lddmm import EPDiff_step, LDDMMAtlasBuilder, expmap, expmap_advect, lddmm_step, shard_indices  # noqa: F401
    from .metric import FluidMetric, FluidMetricOperator, GaussianMetric, Metric  # noqa: F401
    from .points import InterpPointsFunction, deform_points, interp_points, landmark_distance  # noqa: F401
    from .pyramid import (PyramidFunction, image_pyramid, pyramid_expand, pyramid_expand_adjoint,  # noqa: F401
                          pyramid_reduce, pyramid_restrict_adjoint, pyramid_shape)
    from .regularize import (EnergyOperatorFunction, FieldEnergyFunction, bending_energy, diffusion_energy,  # noqa: F401
                             energy_operator, field_energy)
    from .similarity import (JointHistogramFunction, LNCCFunction, LNCCSimilarity, MISimilarity,  # noqa: F401
                             joint_histogram, lncc, lncc_loss, mi_loss, mutual_information)
    from .smooth import GaussianSmoothFunction, gaussian_smooth, gaussian_taps  # noqa: F401

    __version__ = "0.1.0"
