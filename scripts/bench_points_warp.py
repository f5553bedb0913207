"""Time ``tio_points_warp`` (``Engine.warp_points``) against the same solve written with ATen ops, on the same GPU.

    python scripts/bench_points_warp.py [--points 1000000] [--elements 8] [--rounds 3] [--iters 5] [--json out.json]

One launch warps ``elements`` batch elements of ``points`` points each (8 x 10^6 by default: what a tractography or surface
pipeline carries per subject) through the test suite's grids (``tests/annotation_cases.py``: oblique affines, a (5, 7, 6)
control grid at half the folding bound, every element its own matrix and field):
``affine``        no field: ``o = Minv p``;
``elastic``       affine plus field, the Newton solve;
``aten_affine``   ``points.double() @ Minv.T`` per element, rounded to float32;
``aten_elastic``  the same Newton (analytic Jacobian of the trilinear cell, the step halved while the residual does not
                  decrease, the 1e-7 stop, the closing step) as batched float64 tensor ops: every iteration gathers the points
                  that are still active (a read-back of their count, which is what a solve without a kernel of its own has to
                  do to know when to stop), works on them and scatters them back.
Kernel rows are device time per call (events around ``iters`` calls enqueued back to back), ATen rows a host clock around the
call with the device synchronised before and after; the rounds alternate the rows, each row reports the median and the spread.
The ATen ``s`` is also the check: before anything is timed both answers are put back through it (the largest residual over
the converged points) and compared (where the map folds a point has two pre-images; the count of points on which the two
solvers settled on different ones is reported).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import annotation_cases as cases  # noqa: E402
from torchio_amd import ops  # noqa: E402


def device_timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters


def host_timed(fn):
    torch.cuda.synchronize()
    begin = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - begin) * 1e3


def summary(samples):
    ordered = sorted(samples)
    return {"median_ms": round(ordered[len(ordered) // 2], 4), "min_ms": round(ordered[0], 4), "max_ms": round(ordered[-1], 4)}


class AtenMap:
    """One element's ``s`` and Newton solve as float64 tensor ops on the device."""

    def __init__(self, m: cases.Map, device):
        as_tensor = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=device)  # noqa: E731
        self.linear, self.shift = as_tensor(m.matrix[:3, :3]), as_tensor(m.matrix[:3, 3])
        self.inverse, self.inverse_shift = as_tensor(m.inverse[:3, :3]), as_tensor(m.inverse[:3, 3])
        self.field = None if m.field is None else torch.as_tensor(m.field, device=device).double()
        self.affine_first = m.affine_first
        self.in_spacing, self.out_spacing = as_tensor(m.in_spacing), as_tensor(m.out_spacing)
        if self.field is not None:
            self.n = torch.tensor(self.field.shape[:3], device=device)
            self.scale = (self.n - 1).double() / torch.clamp(as_tensor(m.out_shape) - 1.0, min=1.0)

    def s(self, o):
        if self.field is None:
            return o @ self.linear.T + self.shift, self.linear.expand(o.shape[0], 3, 3).clone()
        raw = o * self.scale
        top = (self.n - 1).double()
        inside = (raw >= 0) & (raw <= top)
        u = torch.minimum(torch.clamp(raw, min=0.0), top)
        lo = torch.minimum(u.floor().long(), torch.clamp(self.n - 2, min=0))
        hi = torch.minimum(lo + 1, self.n - 1)
        t = u - lo
        slope = torch.where(inside, self.scale, torch.zeros_like(self.scale))
        pick = lambda x, y, z: self.field[(hi if x else lo)[:, 0], (hi if y else lo)[:, 1], (hi if z else lo)[:, 2]]  # noqa: E731
        w = [(1.0 - t[:, a : a + 1], t[:, a : a + 1]) for a in range(3)]
        vk = {(x, y): pick(x, y, 0) * w[2][0] + pick(x, y, 1) * w[2][1] for x in (0, 1) for y in (0, 1)}
        dk = {(x, y): pick(x, y, 1) - pick(x, y, 0) for x in (0, 1) for y in (0, 1)}
        vj = {x: vk[x, 0] * w[1][0] + vk[x, 1] * w[1][1] for x in (0, 1)}
        dj = {x: vk[x, 1] - vk[x, 0] for x in (0, 1)}
        dkj = {x: dk[x, 0] * w[1][0] + dk[x, 1] * w[1][1] for x in (0, 1)}
        d = vj[0] * w[0][0] + vj[1] * w[0][1]
        derivative = torch.stack([vj[1] - vj[0], dj[0] * w[0][0] + dj[1] * w[0][1], dkj[0] * w[0][0] + dkj[1] * w[0][1]], dim=2) * slope[:, None, :]
        if self.affine_first:
            return o @ self.linear.T + self.shift + d / self.in_spacing, self.linear + derivative / self.in_spacing[:, None]
        inner = torch.eye(3, device=o.device, dtype=torch.float64) + derivative / self.out_spacing[:, None]
        return (o + d / self.out_spacing) @ self.linear.T + self.shift, self.linear @ inner

    def solve(self, points):
        p = points.double()
        o = p @ self.inverse.T + self.inverse_shift
        if self.field is None:
            return o.float()
        s, jacobian = self.s(o)
        err = (s - p).abs().amax(dim=1)
        stalled = torch.zeros_like(err, dtype=torch.bool)
        for _ in range(cases.MAX_ITERATIONS):
            rows = (~(err <= cases.TOLERANCE) & ~stalled).nonzero().squeeze(1)  # (a read-back: tensor ops have to know when to stop)
            if rows.numel() == 0:
                break
            o_r, s_r, j_r, err_r, p_r = o[rows], s[rows], jacobian[rows], err[rows], p[rows]
            step = torch.linalg.solve(j_r, (s_r - p_r).unsqueeze(2)).squeeze(2)
            scale = torch.ones_like(err_r)
            pending = torch.ones_like(err_r, dtype=torch.bool)
            for _ in range(cases.MAX_HALVINGS):
                index = pending.nonzero().squeeze(1)
                if index.numel() == 0:
                    break
                trial = o_r[index] - scale[index, None] * step[index]
                st, jt = self.s(trial)
                et = (st - p_r[index]).abs().amax(dim=1)
                better = et < err_r[index]
                accepted = index[better]
                o_r[accepted], s_r[accepted], j_r[accepted], err_r[accepted] = trial[better], st[better], jt[better], et[better]
                pending[accepted] = False
                scale[pending] *= 0.5
            o[rows], s[rows], jacobian[rows], err[rows] = o_r, s_r, j_r, err_r
            stalled[rows[pending]] = True  # no step length lowered the residual: the best iterate stays
        step = torch.linalg.solve(jacobian, (s - p).unsqueeze(2)).squeeze(2)
        trial = o - step
        better = ((self.s(trial)[0] - p).abs().amax(dim=1) < err) & (err <= cases.TOLERANCE)
        return torch.where(better[:, None], trial, o).float()


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--points", type=int, default=1_000_000)
    parser.add_argument("--elements", type=int, default=8)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--iters", type=int, default=5)
    parser.add_argument("--json", default=None)
    args = parser.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_points_warp.py measures on the GPU; there is none")
    engine = ops.engine()
    device = torch.device("cuda")
    seeds = [11, 15] * ((args.elements + 1) // 2)  # fields on which the float64 reference converges everywhere
    rows = {}
    for kind in ("affine", "elastic"):
        if kind == "affine":
            maps = [cases.Map(cases.voxel_matrix(index + 1), cases.OUT_SHAPE) for index in range(args.elements)]
        else:
            maps = [cases.elastic_map("half_folding", index % 2 == 0, seeds[index]) for index in range(args.elements)]
        generator = torch.Generator(device="cuda").manual_seed(1)
        shape = torch.tensor(cases.IN_SHAPE, device=device, dtype=torch.float32)
        points = (torch.rand((args.elements * args.points, 3), device=device, generator=generator) * 1.2 - 0.1) * (shape - 1)
        offsets = np.arange(args.elements + 1, dtype=np.int64) * args.points
        used, blocks, fields = 0, [], []
        for m in maps:
            blocks.append(m.block(used))
            if m.field is not None:
                fields.append(m.field.reshape(-1))
                used += m.field.size
        blocks_dev = torch.from_numpy(np.stack(blocks)).to(device)
        control = torch.from_numpy(np.concatenate(fields)).to(device) if fields else None
        aten_maps = [AtenMap(m, device) for m in maps]
        pieces = points.split(args.points)
        ours = lambda: engine.warp_points(points, offsets, blocks_dev, control)  # noqa: E731, B023
        theirs = lambda: torch.cat([a.solve(piece) for a, piece in zip(aten_maps, pieces, strict=True)])  # noqa: E731, B023
        moved, status = engine.warp_points(points, offsets, blocks_dev, control, return_status=True)
        baseline = theirs()
        # random points at half the folding bound, a tenth of them outside the grid: where the map folds a point has two
        # pre-images and the two solvers may settle on different ones, so each answer is judged by its own residual under s
        converged = status == 0
        unconverged = int((~converged).sum())
        residuals = []
        for answer in (moved, baseline):
            parts = [(a.s(o.double())[0] - piece.double()).abs().amax(dim=1) for a, o, piece in zip(aten_maps, answer.split(args.points), pieces, strict=True)]
            residuals.append(float(torch.cat(parts)[converged].max()))
        differing = int(((moved - baseline).abs().amax(dim=1) > 1e-3)[converged].sum())
        for _ in range(2):
            ours()
        torch.cuda.synchronize()
        samples = {"kernel": [], "aten": []}
        for _ in range(args.rounds):
            samples["kernel"].append(device_timed(ours, args.iters))
            samples["aten"].append(host_timed(theirs))
        total = args.elements * args.points
        row = {name: summary(values) for name, values in samples.items()}
        row["points"] = total
        row["kernel_mpoints_per_s"] = round(total / row["kernel"]["median_ms"] / 1e3, 1)
        row["kernel_gb_per_s"] = round(total * 24 / row["kernel"]["median_ms"] / 1e6, 1)  # 12 bytes read and 12 written per point
        row["aten_over_kernel"] = round(row["aten"]["median_ms"] / row["kernel"]["median_ms"], 1)
        row["kernel_max_residual"] = float(f"{residuals[0]:.3e}")
        row["aten_max_residual"] = float(f"{residuals[1]:.3e}")
        row["converged_points_on_another_pre_image"] = differing
        row["unconverged"] = unconverged
        rows[kind] = row
        del points, moved, baseline, pieces
        torch.cuda.empty_cache()
    result = {"device": torch.cuda.get_device_name(0), "elements": args.elements, "points_per_element": args.points, "rounds": args.rounds,
              "iters": args.iters, "rows": rows}
    print("| case | kernel ms (min .. max) | Mpoints/s | GB/s | ATen ms (min .. max) | ATen / kernel | max residual kernel / ATen | other pre-image | unconverged |")
    print("|---|---|---|---|---|---|---|---|---|")
    for kind, r in rows.items():
        print(f"| {kind} | {r['kernel']['median_ms']} ({r['kernel']['min_ms']} .. {r['kernel']['max_ms']}) | {r['kernel_mpoints_per_s']} | "
              f"{r['kernel_gb_per_s']} | {r['aten']['median_ms']} ({r['aten']['min_ms']} .. {r['aten']['max_ms']}) | {r['aten_over_kernel']} | "
              f"{r['kernel_max_residual']} / {r['aten_max_residual']} | {r['converged_points_on_another_pre_image']} | {r['unconverged']} |")
    print(json.dumps(result))
    if args.json:
        with open(args.json, "w") as handle:
            json.dump(result, handle, indent=1)


if __name__ == "__main__":
    main()
