"""calodiffusion/utils/HGCal_utils.py of the reference, as far as this package provides it: the geometry maps and converter on
the device, and the pre-processing of HGCal showers at both ends."""
from calodiffusion_amd.hgcal import Decoder, Embeder, HGCalConverter, init_map, load_geom  # noqa: F401
from calodiffusion_amd.postprocess import ReverseNormHGCal  # noqa: F401
from calodiffusion_amd.preprocess import PreprocessHGCal, preprocess_hgcal_shower  # noqa: F401
