from .affine import AffineMatrix
from .aggregator import PatchAggregator
from .batch import ImagesBatch
from .bboxes import BoundingBoxes
from .bboxes import BoundingBoxFormat
from .batch import SubjectsBatch
from .image import Image
from .image import LabelMap
from .image import ScalarImage
from .image import read_image
from .nifti import write_nifti
from .patch import PatchLocation
from .points import Points
from .queue import Queue
from .sampler import GridSampler
from .sampler import LabelSampler
from .sampler import PatchSampler
from .sampler import UniformSampler
from .sampler import WeightedSampler
from .sampler import get_centre_draw
from .sampler import set_centre_draw
from .subject import Subject

__all__ = [
    "AffineMatrix", "BoundingBoxFormat", "BoundingBoxes", "GridSampler", "Image", "ImagesBatch", "LabelMap", "LabelSampler", "PatchAggregator", "PatchLocation",
    "PatchSampler", "Points", "Queue", "ScalarImage", "Subject", "SubjectsBatch", "UniformSampler", "WeightedSampler", "get_centre_draw", "set_centre_draw",
    "read_image", "write_nifti",
]
