"""Run the reference's OWN behavioural tests against torchio_amd (build container only).

    PYTHONDONTWRITEBYTECODE=1 python scripts/run_reference_tests.py [test_blur.py ...]

`torchio` is aliased to `torchio_amd` (package and submodules) and the compute runs on the CPU
oracle through the test-only engine hook, so every test that only needs what this repository
mirrors exercises the mirror's host logic exactly as the reference's authors wrote it.  Nothing
under /root/reference is copied or modified (no bytecode is written; pytest's cache is off).
Tests that need something outside the scope (file I/O, autograd, B-spline orders, other
transforms, private helpers of the reference's implementation) fail or error by design; the
summary at the end is what `tests/REFERENCE_TESTS.md` records.
"""
from __future__ import annotations

import importlib
import importlib.util
import os
import pkgutil
import re
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_TESTS = "/root/reference/tests"
DEFAULT_FILES = [
    "test_blur.py", "test_gamma.py", "test_noise.py", "test_bias_field.py", "test_motion.py", "test_spatial.py", "test_resize.py", "test_anisotropy.py",
    "test_flip.py", "test_pad.py", "test_crop.py", "test_compose.py", "test_one_of.py", "test_some_of.py", "test_inverse.py", "test_parameter_range.py",
    "test_patches.py", "test_queue.py", "test_affine.py", "test_batch.py", "test_per_instance.py", "test_vectorization.py",
    "test_crop_or_pad.py", "test_ensure_shape_multiple.py", "test_to_reference_space.py", "test_copy_affine.py",
    "test_to.py", "test_lambda_transform.py",
    "test_points.py", "test_bboxes.py", "test_axes.py", "test_image_annotations.py", "test_subject.py",
]


# --bound: the seams' own test files plus the containers / protocol files that exercise them through Compose, history, inverse
BOUND_FILES = [
    "test_spatial.py", "test_blur.py", "test_bias_field.py", "test_noise.py", "test_gamma.py", "test_compose.py", "test_inverse.py",
    "test_per_instance.py", "test_vectorization.py",
]


def install_alias() -> None:
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torchio_amd  # noqa: PLC0415
    from oracle.oracle import oracle_engine  # noqa: PLC0415
    from torchio_amd import ops  # noqa: PLC0415

    ops._ENGINE = oracle_engine()
    if importlib.util.find_spec("nibabel") is None:
        # test_crop_or_pad.py imports nibabel at the top and uses it in its file-backed tests only (out of scope: they fail
        # on the empty module); without the name the whole file would not be collected
        sys.modules["nibabel"] = types.ModuleType("nibabel")
    sys.modules["torchio"] = torchio_amd
    for info in pkgutil.walk_packages(torchio_amd.__path__, "torchio_amd."):
        module = importlib.import_module(info.name)
        sys.modules["torchio" + info.name[len("torchio_amd"):]] = module

    # transforms outside the path: the reference's parametrised tests name them at collection
    # time, so the runner (not the product) supplies placeholders whose construction skips that test case
    import pytest  # noqa: PLC0415

    def _placeholder(name):
        common = ("p", "copy", "include", "exclude", "per_instance")

        def __init__(self, *args, **kwargs):
            torchio_amd.transforms.Transform.__init__(self, **{k: v for k, v in kwargs.items() if k in common})

        def skip(self, *args, **kwargs):
            pytest.skip(f"{name} is not part of the hot path (SURVEY section 8)")

        return type(name, (torchio_amd.transforms.Transform,), {"__init__": __init__, "forward": skip, "make_params": skip})

    # Ghosting, Spike, Swap and LabelsToImage exist in the package, but this run computes on the CPU oracle, which has no
    # counterpart of their HIP-only entry points (those are checked on the GPU, tests/test_gpu_kspace_artefacts.py,
    # tests/test_gpu_swap_histogram.py and tests/test_gpu_labels_to_image.py): the placeholders stay whatever is exported.
    # Reorient and Transpose move their voxels with tio_permute3d, HIP-only as well (tests/test_gpu_orientation.py), and
    # the reference's test_reorient.py needs the real nibabel.
    for hip_only in ("Ghosting", "Spike", "Swap", "LabelsToImage", "Reorient", "Transpose"):
        setattr(torchio_amd, hip_only, _placeholder(hip_only))

    # the reference keeps its spatial transforms in a package (torchio.transforms.spatial.spatial); private helpers
    # with no counterpart here (the sampling grid is never materialised ...) resolve to a stub that raises when called
    import torchio_amd.transforms.spatial as real  # noqa: PLC0415

    class Shim(types.ModuleType):
        def __getattr__(self, item):
            if hasattr(real, item):
                return getattr(real, item)

            def missing(*args, **kwargs):
                raise NotImplementedError(f"{item} is an internal of the reference with no counterpart")

            return missing

    package = types.ModuleType("torchio.transforms.spatial")
    package.__path__ = []
    for key, value in vars(real).items():
        setattr(package, key, value)
    sys.modules["torchio.transforms.spatial"] = package
    sys.modules["torchio.transforms.spatial.spatial"] = Shim("torchio.transforms.spatial.spatial")
    for name in ("anisotropy", "resize", "flip", "pad"):  # flat modules here, members of the spatial package there
        sys.modules[f"torchio.transforms.spatial.{name}"] = importlib.import_module(f"torchio_amd.transforms.{name}")
    sys.modules["torchio.transforms.spatial.crop"] = sys.modules["torchio.transforms.spatial.pad"]  # Pad and Crop share a module
    sys.modules["torchio.transforms.spatial._padding"] = sys.modules["torchio.transforms.spatial.pad"]
    orientation = importlib.import_module("torchio_amd.transforms.orientation")  # six classes of the spatial package, one module here
    for name in ("crop_or_pad", "ensure_shape_multiple", "to_reference_space", "copy_affine", "reorient", "transpose"):
        sys.modules[f"torchio.transforms.spatial.{name}"] = orientation


def install_binding() -> None:
    """--bound: the REAL reference package with `torchio_amd.reference_binding` applied, compute on the CPU oracle —
    the reference's own classes, containers and tests; only the five seams run this repository's code."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import ref_import  # noqa: PLC0415
    from oracle.oracle import oracle_engine  # noqa: PLC0415
    from torchio_amd import ops  # noqa: PLC0415
    from torchio_amd import reference_binding  # noqa: PLC0415

    reference = ref_import.import_reference()
    ops._ENGINE = oracle_engine()
    reference_binding.bind(reference)


def run_one(name: str, bound: bool = False) -> int:
    import pytest  # noqa: PLC0415

    if bound:
        install_binding()
    else:
        install_alias()
    return pytest.main(["-p", "no:cacheprovider", "-q", "--rootdir=/tmp", "-W", "ignore", os.path.join(REFERENCE_TESTS, name)])


def main() -> None:
    if len(sys.argv) == 3 and sys.argv[1] in ("--one", "--one-bound"):
        sys.exit(run_one(sys.argv[2], bound=sys.argv[1] == "--one-bound"))
    bound = "--bound" in sys.argv[1:]
    files = [arg for arg in sys.argv[1:] if arg != "--bound"] or (BOUND_FILES if bound else DEFAULT_FILES)
    rows = []
    for name in files:
        env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
        result = subprocess.run([sys.executable, __file__, "--one-bound" if bound else "--one", name], capture_output=True, text=True, env=env, cwd="/tmp")
        tail = result.stdout.strip().splitlines()[-1] if result.stdout.strip() else result.stderr.strip().splitlines()[-1]
        counts = {key: int(value) for value, key in re.findall(r"(\d+) (passed|failed|skipped|errors|error)", tail)}
        failed = [line.split(" - ")[0].replace("FAILED ::", "") for line in result.stdout.splitlines() if line.startswith("FAILED")]
        rows.append((name, counts, failed))
        print(f"{name:28s} {tail}")
    print()
    print("| file | passed | failed / error | failing tests |")
    print("|---|---|---|---|")
    for name, counts, failed in rows:
        bad = counts.get("failed", 0) + counts.get("error", 0) + counts.get("errors", 0)
        print(f"| `{name}` | {counts.get('passed', 0)} | {bad} | {', '.join(failed) if failed else ''} |")


if __name__ == "__main__":
    main()
