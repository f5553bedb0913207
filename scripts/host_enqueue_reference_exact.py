"""Host enqueue time per step of the bench pipeline in the reference,exact mode — the mode that runs ``HostNormalStream`` every
step; bench.py's mode matrix reports its volumes/s but no host time.  ``argv[1]``: the tree to import ``bench`` and
``torchio_amd`` from (default: this one), so that two checkouts can be alternated on one box.  Prints one JSON line: three
blocks of 30 steps per draw policy ("off", the library default, and "gated", the draw-stream road)."""
import importlib.util
import json
import os
import sys
import time

root = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
spec = importlib.util.spec_from_file_location("bench", os.path.join(root, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)  # (puts its own tree in front of sys.path)

import torch  # noqa: E402

import torchio_amd as tio  # noqa: E402

assert os.path.abspath(tio.__file__).startswith(root), (tio.__file__, root)
device = torch.device("cuda", 0)
torch.cuda.set_device(device)
transform = bench.build_transform()
batch = bench.make_batch(256, 8, 1234, device)
tio.set_noise_rng("reference")
tio.set_resample_precision("exact")
tio.set_stencil_precision("exact")
result = {"tree": root}
for policy in ("off", "gated"):
    tio.set_draw_policy(policy)
    torch.manual_seed(77)
    out = None
    for _ in range(40):
        out = transform(batch)
    torch.cuda.synchronize()
    host, total = [], []
    for _ in range(3):
        start = time.perf_counter()
        for _ in range(30):
            out = transform(batch)
        enqueue = time.perf_counter() - start
        torch.cuda.synchronize()
        total.append(round(1e3 * (time.perf_counter() - start) / 30, 4))
        host.append(round(1e3 * enqueue / 30, 4))
    result[policy] = {"host_enqueue_ms_per_step": host, "ms_per_step": total}
print(json.dumps(result))
