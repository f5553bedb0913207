"""Axis strings of annotations (mirror of reference ``data/axes.py``).

Three upper-case letters name the order and direction of a coordinate system: a permutation of ``"IJK"`` (voxel indices) or
one letter of each anatomical pair R/L, A/P, S/I in any order (world millimetres).  ``"IJK"`` always means voxels.
"""
from __future__ import annotations

from enum import Enum

ANATOMICAL_PAIRS: tuple[tuple[str, str], ...] = (("R", "L"), ("A", "P"), ("S", "I"))
#: letter -> index of its pair
_PAIR_OF = {letter: index for index, pair in enumerate(ANATOMICAL_PAIRS) for letter in pair}


class AxesType(Enum):
    """Voxel or anatomical coordinates."""

    VOXEL = "voxel"
    ANATOMICAL = "anatomical"


def _is_voxel(axes: str) -> bool:
    return len(axes) == 3 and sorted(axes) == ["I", "J", "K"]


def _is_anatomical(axes: str) -> bool:
    return len(axes) == 3 and all(c in _PAIR_OF for c in axes) and sorted(_PAIR_OF[c] for c in axes) == [0, 1, 2]


def validate_axes(axes: str) -> str:
    """*axes* itself when it is a valid axis string, ``ValueError`` otherwise."""
    if len(axes) != 3:
        raise ValueError(f"Axis string must be 3 characters, got {len(axes)}: {axes!r}")
    if _is_voxel(axes) or _is_anatomical(axes):
        return axes
    raise ValueError(
        f"Invalid axis string {axes!r}. Must be a permutation of 'IJK' (voxel) or one letter from each anatomical pair"
        " {R,L}, {A,P}, {S,I}."
    )


def axes_type(axes: str) -> AxesType:
    """The family of an already validated axis string."""
    return AxesType.VOXEL if _is_voxel(axes) else AxesType.ANATOMICAL


def get_axis_mapping(src: str, tgt: str) -> tuple[tuple[int, int, int], tuple[bool, bool, bool]]:
    """``(permutation, flips)`` from *src* to *tgt* (same family): target column ``c`` is source column ``permutation[c]``,
    negated where ``flips[c]``."""
    src_type, tgt_type = axes_type(src), axes_type(tgt)
    if src_type != tgt_type:
        raise ValueError(
            f"Cannot compute axis mapping between different types: {src!r} ({src_type.value}) and {tgt!r} ({tgt_type.value})."
            " Use the affine to convert between voxel and anatomical. Both must be the same type."
        )
    if src_type == AxesType.VOXEL:
        perm = tuple(src.index(letter) for letter in tgt)
        return (perm[0], perm[1], perm[2]), (False, False, False)
    pairs = [_PAIR_OF[letter] for letter in src]
    perm = tuple(pairs.index(_PAIR_OF[letter]) for letter in tgt)
    flips = tuple(src[column] != letter for column, letter in zip(perm, tgt, strict=True))
    return (perm[0], perm[1], perm[2]), (flips[0], flips[1], flips[2])
