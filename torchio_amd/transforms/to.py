"""``To``: a device move or dtype cast as a pipeline step (mirror of reference ``transforms/to.py``)."""
from __future__ import annotations

from typing import Any

from ..data.batch import SubjectsBatch
from .transform import Transform


class To(Transform):
    """``batch.to(*to_args, **to_kwargs)`` on every image of the batch: a device (``"cuda"``), a dtype (``torch.float16``),
    or whatever else ``torch.Tensor.to`` takes.  The arguments are the recorded parameters."""

    def __init__(self, *to_args: Any, **to_kwargs: Any) -> None:
        super().__init__()
        self.to_args = to_args
        self.to_kwargs = to_kwargs

    def make_params(self, batch: SubjectsBatch) -> dict[str, Any]:
        return {"to_args": self.to_args, "to_kwargs": self.to_kwargs}

    def apply_transform(self, batch: SubjectsBatch, params: dict[str, Any]) -> SubjectsBatch:
        batch.to(*params["to_args"], **params["to_kwargs"])
        return batch
