"""calodiffusion/train/evaluate.py of the reference: the Frechet physics distance objective, its moments computed on the device
(ComparisonNetwork and CNNCompare, which need torchvision, are not provided)."""
from calodiffusion_amd.evaluate import FDP, FDPCalculationError  # noqa: F401
