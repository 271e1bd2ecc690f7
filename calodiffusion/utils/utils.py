"""calodiffusion/utils/utils.py of the reference, as far as the hot path uses it: device choice, coordinate images, load_attr,
ReverseNorm, preprocess_shower, the Dataset-1
geometry converters."""
from calodiffusion_amd.utils import *  # noqa: F401,F403
from calodiffusion_amd.utils import create_phi_image, create_R_Z_image, get_device, load_attr, subsample_alphas  # noqa: F401
from calodiffusion_amd.postprocess import ReverseNorm, ReverseNormCaloChall  # noqa: F401
from calodiffusion_amd.preprocess import Preprocess, PreprocessDS1, preprocess_shower  # noqa: F401
from calodiffusion_amd.geom1 import GeomConverter, NNConverter  # noqa: F401
from calodiffusion_amd.xml_handler import XMLHandler  # noqa: F401
