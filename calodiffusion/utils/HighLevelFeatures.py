"""calodiffusion/utils/HighLevelFeatures.py of the reference: the CaloChallenge shower observables, computed on the device."""
from calodiffusion_amd.hlf import HighLevelFeatures  # noqa: F401
