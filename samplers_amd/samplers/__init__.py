from .base import PosteriorSampler
from .ddrm import DDRMSampler, FusedDDRMStep, ddrm_step_svd
from .diffpir import DiffPIRSampler, FusedDiffPIRStep
from .dps import DPSSampler, FusedDPSStep, KernelTimer
from .pgdm import PGDMSampler
from .psld import FusedPSLDStep, PSLDSampler
from .resample import ReSampleSampler

__all__ = ["PosteriorSampler", "DPSSampler", "PSLDSampler", "PGDMSampler", "ReSampleSampler",
           "DiffPIRSampler", "DDRMSampler", "FusedDPSStep", "FusedDiffPIRStep", "FusedDDRMStep",
           "FusedPSLDStep", "KernelTimer", "ddrm_step_svd"]
