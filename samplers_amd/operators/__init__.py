from .base import NonlinearOperator, Operator
from .blur import GaussianBlurOperator
from .channel_mix import ChannelMixOperator
from .hadamard import HadamardOperator
from .identity import IdentityOperator
from .inpainting import (
    CenterInpaintingOperator,
    CenterOutpaintingOperator,
    InpaintingOperator,
    RandomInpaintingOperator,
    SidePaintingOperator,
    get_mask_inpaint_center,
    get_mask_random,
    get_mask_side_painting,
)
from .phase import PhaseRetrievalOperator
from .linear import GeneralSVDOperator, LinearOperator, SVDOperator
from .psf import MotionBlurOperator, PSFBlurOperator, motion_blur_kernel
from .periodic import PeriodicBlurOperator, pseudo_inverse_spectrum, transfer_function
from .psf_fft import FFTPSFBlurOperator, padded_size, psf_spectrum
from .radon import RadonOperator, radon_table
from .sr_filter import BicubicSuperResolutionOperator, FilteredSuperResolutionOperator, bicubic_taps
from .sr_periodic import PeriodicSuperResolutionOperator
from .superres import SuperResolutionOperator
from .svd_separable import SeparableSVDOperator

__all__ = [
    "Operator",
    "NonlinearOperator",
    "IdentityOperator",
    "LinearOperator",
    "GeneralSVDOperator",
    "SVDOperator",
    "InpaintingOperator",
    "CenterInpaintingOperator",
    "CenterOutpaintingOperator",
    "SidePaintingOperator",
    "RandomInpaintingOperator",
    "GaussianBlurOperator",
    "SuperResolutionOperator",
    "FilteredSuperResolutionOperator",
    "BicubicSuperResolutionOperator",
    "PeriodicSuperResolutionOperator",
    "bicubic_taps",
    "PSFBlurOperator",
    "MotionBlurOperator",
    "FFTPSFBlurOperator",
    "PeriodicBlurOperator",
    "SeparableSVDOperator",
    "HadamardOperator",
    "ChannelMixOperator",
    "PhaseRetrievalOperator",
    "RadonOperator",
    "radon_table",
    "motion_blur_kernel",
    "padded_size",
    "psf_spectrum",
    "transfer_function",
    "pseudo_inverse_spectrum",
    "get_mask_inpaint_center",
    "get_mask_side_painting",
    "get_mask_random",
]
