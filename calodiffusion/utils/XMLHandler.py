"""calodiffusion/utils/XMLHandler.py of the reference: the binning-file reader."""
from calodiffusion_amd.xml_handler import XMLHandler  # noqa: F401
