"""Record what ``tio_resample3d_plan_bytes`` answers for the route table of ``tests/test_plan_bytes_routes.py``.

Run on a checkout whose library is the one to pin (no GPU needed; build first):

    python tests/golden/make_plan_bytes_routes.py      # writes tests/golden/plan_bytes_routes.json

The file was recorded from the dispatcher as it stood before it was split into route choice and launch helpers; a change
that moves one of these integers moves a call to another road (or another plan layout) and has to say so.
Test infrastructure: nothing under ``torchio_amd/`` imports this file.
"""
from __future__ import annotations

import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests.test_plan_bytes_routes import CASES, GOLDEN, plan_bytes  # noqa: E402


def main() -> None:
    recorded = {case_id: plan_bytes(case_id) for case_id in sorted(CASES)}
    with open(GOLDEN, "w", encoding="utf-8") as handle:
        json.dump(recorded, handle, indent=0, sort_keys=True)
        handle.write("\n")
    zero = sum(1 for v in recorded.values() if v == 0)
    print(f"{len(recorded)} cases, {zero} without a plan -> {GOLDEN}")


if __name__ == "__main__":
    main()
