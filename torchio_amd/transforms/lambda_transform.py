"""``Lambda``: a user's callable as a pipeline step (mirror of reference ``transforms/lambda_transform.py``)."""
from __future__ import annotations

from collections.abc import Callable
from typing import Any

from torch import Tensor

from ..data import _lazy
from ..data.batch import SubjectsBatch
from ..data.image import LabelMap
from ..data.image import ScalarImage
from .transform import Transform

_CLASS_OF_TYPE = {"scalar": ScalarImage, "label": LabelMap}


class Lambda(Transform):
    """Call ``function`` on each batch element's ``(C, I, J, K)`` device tensor and assign what it returns into that
    element: the batch keeps its dtype, and a result of another shape raises torch's own error.  ``types_to_apply``:
    ``"scalar"`` for scalar images only, ``"label"`` for label maps only, ``None`` for every image.  As in the reference
    the word is not validated: any other value applies the function to every image, like ``None``."""

    def __init__(self, function: Callable[[Tensor], Tensor], types_to_apply: str | None = None, **kwargs: Any) -> None:
        super().__init__(**kwargs)
        if not callable(function):
            raise TypeError(f"function must be callable, got {type(function).__name__}")
        self.function = function
        self.types_to_apply = types_to_apply

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {}

    def _should_apply(self, image_class: type) -> bool:
        wanted = _CLASS_OF_TYPE.get(self.types_to_apply)
        return wanted is None or issubclass(image_class, wanted)

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        for img_batch in batch.images.values():
            if not self._should_apply(img_batch._image_class):
                continue
            # .data launches whatever an earlier transform deferred: the callable sees finished values.  The elements are
            # written in place, as in the reference; only a tensor the batch still shares with the caller (copy-on-replace,
            # data/_lazy.py) is cloned first.  With copy=False the caller's tensor is written, as the reference does.
            data = img_batch.data
            if _lazy.is_borrowed(img_batch):
                data = data.clone()
                img_batch.data = data
            for index in range(img_batch.batch_size):
                data[index] = self.function(data[index])
        return batch
