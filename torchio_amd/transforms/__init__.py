from .anisotropy import Anisotropy
from .bias_field import BiasField
from .blur import Blur
from .compose import Compose
from .compose import OneOf
from .compose import SomeOf
from .flip import Flip
from .gamma import Gamma
from .ghosting import Ghosting
from .histogram_standardization import HistogramStandardization
from .inverse import apply_inverse_transform
from .inverse import get_inverse_transform
from .lambda_transform import Lambda
from .labels import Contour
from .labels import KeepLargestComponent
from .labels import OneHot
from .labels import RemapLabels
from .labels import RemoveLabels
from .labels import SequentialLabels
from .labels_to_image import LabelsToImage
from .motion import Motion
from .noise import Noise
from .noise import get_noise_rng
from .noise import set_noise_rng
from .normalize import Clamp
from .normalize import Mask
from .normalize import Normalize
from .normalize import RescaleIntensity
from .normalize import Standardize
from .normalize import ZNormalization
from .orientation import CopyAffine
from .orientation import CropOrPad
from .orientation import EnsureShapeMultiple
from .orientation import Reorient
from .orientation import ToReferenceSpace
from .orientation import Transpose
from .pad import Crop
from .pad import Pad
from .parameter_range import Choice
from .pca import PCA
from .resize import Resize
from .spatial import Affine
from .spatial import ElasticDeformation
from .spatial import Resample
from .spatial import Spatial
from .spike import Spike
from .swap import Swap
from .to import To
from .transform import AppliedTransform
from .transform import IntensityTransform
from .transform import SpatialTransform
from .transform import Transform

__all__ = [
    "Affine", "Anisotropy", "AppliedTransform", "BiasField", "Blur", "Choice", "Clamp", "Compose", "Contour", "CopyAffine", "Crop", "CropOrPad", "ElasticDeformation", "EnsureShapeMultiple", "Flip", "Gamma", "Ghosting",
    "HistogramStandardization", "IntensityTransform", "KeepLargestComponent", "LabelsToImage", "Lambda", "Mask", "Motion", "Noise", "Normalize", "OneHot", "OneOf", "PCA", "Pad", "RemapLabels", "RemoveLabels", "Reorient", "Resample", "RescaleIntensity",
    "Resize", "SequentialLabels", "SomeOf", "Spatial", "SpatialTransform", "Spike", "Standardize", "Swap", "To", "ToReferenceSpace", "Transform", "Transpose", "ZNormalization",
    "apply_inverse_transform", "get_inverse_transform", "get_noise_rng", "set_noise_rng",
]
