"""GPU: the ordering BETWEEN streams, under forced delays (tests/stream_holds.py).

The library hands buffers across streams in several places — the ahead stream of `Spatial._prefetch`, the draw stream of the
reference's noise, the pinned rings behind `non_blocking` uploads, the per-stream workspaces inside libtio_hip.so, and the
caller's own protocol for a plan made ahead.  On an idle GPU the producer is always done before the consumer gets there, so
a missing `wait_event` or `record_stream`, or a buffer reused one upload too early, changes nothing one could compare.  Here
one side is HELD (a kernel that keeps a stream busy and ends by itself) while the other enqueues, in both directions:

* producer late: the side stream is held before the step; the consumer's stream is free and really independent of it
  (`independent_stream`: the teeth probe on plain torch ops);
* consumer late: the data stream is held and six steps are issued back to back, so that the side streams and the caching
  allocators run steps ahead.

Numerics are pinned elsewhere.  What is expected here comes from the plainest mode — no ahead stream, draw policy "off", the
device synchronised after every step — and must be met bit for bit: outputs, the applied-transform history, the global
generator's state.  That a run was really made under a hold is an assertion too: every watched consumer launch was enqueued
while the hold was still in force (a hold lasts four times what the host needed to enqueue the same work in the plain pass,
at least 20 ms, at most 500 ms; if that cap is too short the assertion fails and says so).

Nothing here switches the library's ordering off to show that a test can fail: that would launch kernels on unwritten plans.
The sensitivity check is the teeth probe, together with the in-force assertions.

`TIO_STREAM_ORDER_REPORT=<path>` writes the calibration of the hold, the chosen stream pairs, the measured enqueue times
and the hold lengths there (profiles/stream_order.md is such a report).
"""
from __future__ import annotations

import copy
import os
import threading
import warnings

import pytest
import torch

import stream_holds as sh
import torchio_amd as tio
from test_gpu_ops_parity import _control_points
from test_gpu_ops_parity import _mapping
from test_gpu_resample_planned import starts_from_a_plan
from test_gpu_resample_planned import two_thread_jobs
from torchio_amd import noise_stream
from torchio_amd import ops
from torchio_amd import streams

pytestmark = pytest.mark.gpu

STEPS = 6
ROWS: list[dict] = []  # one per held run: what the report lists


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("TIO_STREAM_ORDER_REPORT")
    if not path or not ROWS:
        return
    lines = ["# Stream ordering under forced delays: what tests/test_gpu_stream_order.py measured", ""]
    lines += ["## The hold primitive", ""]
    for device, record in sh.CALIBRATION.items():
        shown = {key: value for key, value in record.items() if key != "buffer"}
        lines.append(f"- device {device}: {shown}")
    lines += ["", "## Stream pairs the teeth probe chose (held stream -> a stream that runs beside it)", ""]
    for pair in sh.PAIRS:
        lines.append(f"- held {pair['side']:#x} -> free {pair['chosen']:#x} (candidate {pair['candidates_tried']}): {pair['probe']}")
    lines += ["", "## Held runs", "", "| scenario | direction | plain enqueue (ms) | hold (ms) | held stream | consumer stream | watched launches in force | held run: enqueue per step (ms) |",
              "|---|---|---|---|---|---|---|---|"]
    for row in ROWS:
        lines.append(f"| {row['scenario']} | {row['direction']} | {row['enqueue_ms']:.2f} | {row['hold_ms']:.1f} | {row['held']:#x} | {row['consumer']:#x} | {row['in_force']} | {row['steps_ms']} |")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", encoding="utf-8") as file:
        file.write("\n".join(lines) + "\n")


@pytest.fixture
def modes():
    """The library's process-wide modes, put back whatever a test set."""
    previous = (tio.get_noise_rng(), tio.get_resample_precision(), tio.get_stencil_precision(), ops.get_draw_policy(), ops.get_noise_plan(),
                streams._AHEAD_ENABLED)
    yield
    tio.set_noise_rng(previous[0])
    tio.set_resample_precision(previous[1])
    tio.set_stencil_precision(previous[2])
    ops.set_draw_policy(previous[3])
    ops.set_noise_plan(previous[4])
    ops.set_ahead_stream(previous[5])
    ops.expect_minimum_fill(False)


def _row(scenario, direction, enqueue_ms, held, consumer, in_force, steps_ms=None) -> None:
    ROWS.append(dict(scenario=scenario, direction=direction, enqueue_ms=enqueue_ms, hold_ms=held.ms, held=held.stream.stream_id,
                     consumer=consumer.stream_id, in_force=in_force, steps_ms="" if steps_ms is None else " ".join(f"{ms:.2f}" for ms in steps_ms)))


def _assert_in_force(calls, held, what: str) -> str:
    """Every one of *calls* (`Watch.of`) was enqueued while *held* was in force; returns "n of n" for the report."""
    assert calls, f"{what}: no watched launch was recorded"
    inside = [call[2][held.label] for call in calls]
    assert all(inside), (
        f"{what}: launches enqueued after the hold of {held.ms:.0f} ms had ended: {inside} — the run proves nothing about ordering"
        + (f" (the cap of {sh.MAX_HOLD_MS:.0f} ms is too short for this host)" if held.ms >= sh.MAX_HOLD_MS else "")
    )
    return f"{sum(inside)} of {len(inside)}"


# ---------------------------------------------------------------------------------------------------------------------
# pipelines: (a) the ahead stream, (b) the draw stream
# ---------------------------------------------------------------------------------------------------------------------
def _history(out):
    return [(t.name, copy.deepcopy(dict(t.params))) for t in out.applied_transforms]


def _run_pipeline(make_pipeline, source, steps, *, stream, sync_each, watch_names=(), before=None):
    """*steps* passes of a fresh pipeline over *source* on *stream*, seeded alike every time.  Returns the outputs per step
    (image tensors, history, the global generator's state behind the step), a `torch.rand(3)` probe of the generator behind
    the last step, the host's enqueue time per step (ms) and the watch.  *before(watch)*: called right before the first
    step, on the host (where a run puts its hold)."""
    pipeline = make_pipeline()
    assert pipeline._may_draw_ahead()
    torch.manual_seed(23)
    results, states, enqueue_ms = [], [], []
    with sh.watch(ops.engine(), watch_names) as watch, torch.cuda.stream(stream), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if before is not None:
            before(watch)
        for _ in range(steps):
            clock = sh.Stopwatch()
            clock.start()
            out = pipeline(source)
            tensors = {name: image.data for name, image in out.images.items()}  # (reading `.data` enqueues whatever is still queued)
            clock.stop()
            enqueue_ms.append(clock.ms)
            states.append(torch.get_rng_state())
            results.append((tensors, out))
            if sync_each:
                torch.cuda.synchronize()
    probe = torch.rand(3)
    torch.cuda.synchronize()
    steps_out = [(tensors, _history(out), state) for (tensors, out), state in zip(results, states, strict=True)]
    return steps_out, probe, enqueue_ms, watch


def _assert_same_steps(got, expected, what: str) -> None:
    for index, (a, b) in enumerate(zip(got, expected)):  # (a one-step run is compared with the first expected step)
        assert a[0].keys() == b[0].keys()
        for name in a[0]:
            assert torch.equal(a[0][name], b[0][name]), f"{what}: image {name!r} of step {index} differs from the plain pass"
        assert a[1] == b[1], f"{what}: the history of step {index} differs"
        assert torch.equal(a[2], b[2]), f"{what}: the global generator's state behind step {index} differs"


_PLAIN: dict = {}  # scenario key -> the plain pass (computed once, shared by both directions and every policy, never written)


def _plain_pass(key, make_pipeline, source, stream):
    """The expected values of a pipeline scenario: no ahead stream, draw policy "off", a synchronisation behind every step.
    One pass before the timed one warms the caches, so that the enqueue times it reports are those of a warm host."""
    if key not in _PLAIN:
        ops.set_ahead_stream(False)
        ops.set_draw_policy("off")
        _run_pipeline(make_pipeline, source, 1, stream=stream, sync_each=True)
        steps_out, probe, enqueue_ms, _ = _run_pipeline(make_pipeline, source, STEPS, stream=stream, sync_each=True)
        _PLAIN[key] = (steps_out, probe, enqueue_ms)
    return _PLAIN[key]


AHEAD_SHAPE = (68, 72, 80)  # K % 4 == 0, 16-byte rows, and every axis >= 16 * 4 + 1: a 5^3 control grid's cells span a brick


def _ahead_source():
    g = torch.Generator().manual_seed(17)
    subjects = [
        tio.Subject(t1=tio.ScalarImage(torch.rand(1, *AHEAD_SHAPE, generator=g)),
                    seg=tio.LabelMap(torch.randint(0, 4, (1, *AHEAD_SHAPE), generator=g, dtype=torch.int16)))
        for _ in range(2)
    ]
    source = tio.SubjectsBatch.from_subjects(subjects).to("cuda")
    torch.cuda.synchronize()
    return source


def _ahead_pipeline():
    return tio.Compose([
        tio.Affine(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5)),
        tio.ElasticDeformation(num_control_points=5),
    ])


AHEAD_ROADS = {"fast": ("TIO_FAST_KERNEL", "planned"), "exact": ("TIO_EXACT_LEAN", "2")}


@pytest.mark.parametrize("direction", ["producer late", "consumer late"])
@pytest.mark.parametrize("precision", ["fast", "exact"])
def test_ahead_stream_hands_over_in_order(hip, modes, monkeypatch, precision, direction):
    """(a) `Spatial._prefetch` uploads mapping, control points and flags and makes the brick plan on the ahead stream;
    `Ahead.join` orders the data stream behind them.  Compose[Affine, ElasticDeformation(5 control points)] on 2 x (float32
    image + int16 label map) of 68 x 72 x 80, forced onto the planned roads — asserted: the plans are made, on the ahead stream."""
    monkeypatch.setenv(*AHEAD_ROADS[precision])
    tio.set_resample_precision(precision, allow_out_of_tolerance=True)
    device = torch.device("cuda", torch.cuda.current_device())
    ops.set_ahead_stream(True)
    side = streams.ahead_stream(device)
    data_stream = sh.independent_stream(side, device, keep=True)
    source = _ahead_source()
    # the road is the planned one, for the affine and for the elastic launch of this geometry
    geometry = dict(out_shape=AHEAD_SHAPE, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True)
    mapping = torch.eye(3, 4).repeat(2, 1, 1).cuda()
    field = torch.zeros(2, 5, 5, 5, 3, device="cuda")
    assert starts_from_a_plan(hip, [source.t1.data], precision=precision, mapping=mapping, control_points=None, **geometry)
    assert starts_from_a_plan(hip, [source.t1.data], precision=precision, mapping=mapping, control_points=field, **geometry)
    expected, probe, enqueue_ms = _plain_pass(("ahead", precision), _ahead_pipeline, source, data_stream)

    ops.set_ahead_stream(True)
    steps = 1 if direction == "producer late" else STEPS
    plain_ms = sum(enqueue_ms[:steps])
    holds = []

    def before(watch):
        held_stream = side if direction == "producer late" else data_stream
        holds.append(watch.add(sh.hold(held_stream, sh.hold_length(plain_ms), direction)))

    got, got_probe, held_ms, watch = _run_pipeline(_ahead_pipeline, source, steps, stream=data_stream, sync_each=False,
                                                   watch_names=("resample3d", "resample3d_plan", "channel_min"), before=before)
    held = holds[0]
    plans = watch.of("resample3d_plan")
    assert len(plans) == 2 * steps and all(call[1] == side.stream_id for call in plans), plans  # both children plan, on the ahead stream
    launches = watch.of("resample3d", data_stream)
    assert len(launches) == len(watch.of("resample3d")) == 2 * steps
    in_force = _assert_in_force(launches, held, f"ahead stream, {precision}, {direction}")
    _row(f"(a) ahead stream, {precision}", direction, plain_ms, held, data_stream, in_force, held_ms)
    _assert_same_steps(got, expected, f"ahead stream, {precision}, {direction}")
    if steps == STEPS:
        assert torch.equal(got_probe, probe)


def test_cached_identity_mapping_is_written_before_another_stream_reads_it(hip, modes):
    """(a) A purely elastic launch maps through ONE cached identity tensor per device, uploaded by whoever asks first — in a
    Compose that draws ahead that is `_prefetch`, on the ahead stream, and `Ahead.join` orders only that Compose's own launch
    behind it.  With the ahead stream held and the cache empty (as in a fresh process), a Compose on one stream is followed at
    once by a plain ElasticDeformation on ANOTHER stream, which joins nothing: it must find the mapping written."""
    from torchio_amd.transforms import spatial as sp

    device = torch.device("cuda", torch.cuda.current_device())
    ops.set_ahead_stream(True)
    side = streams.ahead_stream(device)
    first = sh.independent_stream(side, device, keep=True)
    second = sh.independent_stream(side, device, avoid=(first,))
    source = _ahead_source()

    def run():
        torch.manual_seed(5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with torch.cuda.stream(first):
                composed = tio.Compose([tio.ElasticDeformation(num_control_points=5), tio.ElasticDeformation(num_control_points=5)])(source)
            with torch.cuda.stream(second):
                alone = tio.ElasticDeformation(num_control_points=5)(source)
        return [image.data for out in (composed, alone) for image in out.images.values()]

    ops.set_ahead_stream(False)
    expected = run()
    torch.cuda.synchronize()
    ops.set_ahead_stream(True)
    sp._IDENTITY_MAPPINGS.clear()
    held = sh.hold(side, sh.FLOOR_HOLD_MS, "identity")
    got = run()
    torch.cuda.synchronize()
    assert str(device) in sp._IDENTITY_MAPPINGS  # the launches did go through the cached tensor
    _row("(a) cached identity mapping", "producer late", 0.0, held, second, "n/a (the first upload waits for its stream on the host)")
    for index, (a, b) in enumerate(zip(expected, got, strict=True)):
        assert torch.equal(a, b), f"tensor {index} differs from the run without the ahead stream"


DRAW_SHAPE = (64, 64, 128)  # 2 x 1 x 64 x 64 x 128 = 2^20 draws: exactly DEVICE_DRAW_MIN, the smallest batch the draw stream takes


def _draw_source():
    g = torch.Generator().manual_seed(29)
    subjects = [tio.Subject(t1=tio.ScalarImage(torch.rand(1, *DRAW_SHAPE, generator=g))) for _ in range(2)]
    source = tio.SubjectsBatch.from_subjects(subjects).to("cuda")
    torch.cuda.synchronize()
    return source


def _draw_pipeline():
    return tio.Compose([
        tio.Affine(degrees=(-10, 10), scales=(0.9, 1.1), translation=(-5, 5)),
        tio.Blur(std=(0.5, 1.5)),
        tio.Noise(std=(0.02, 0.05)),
    ])


@pytest.mark.parametrize("direction", ["producer late", "consumer late"])
@pytest.mark.parametrize("policy", ["gated", "free"])
def test_draw_stream_hands_over_in_order(hip, modes, policy, direction):
    """(b) The reference's noise draws are made on the low-priority draw stream (`on_draw_stream`: the gate of the "gated"
    policy, the host back-pressure of four draws in flight, the hand-over event) and consumed by the fused stencil launch of
    the data stream.  Compose[Affine, Blur, Noise], reference noise, 2^20 draws per step."""
    assert 2 * DRAW_SHAPE[0] * DRAW_SHAPE[1] * DRAW_SHAPE[2] == ops.HostNormalStream.DEVICE_DRAW_MIN
    tio.set_noise_rng("reference")
    device = torch.device("cuda", torch.cuda.current_device())
    ops.set_ahead_stream(True)
    ops.set_draw_policy(policy)
    side = streams.draw_stream(device)
    assert side is not None
    data_stream = sh.independent_stream(side, device, keep=True)
    source = _draw_source()
    expected, probe, enqueue_ms = _plain_pass(("draw",), _draw_pipeline, source, data_stream)

    ops.set_ahead_stream(True)
    ops.set_draw_policy(policy)
    steps = 1 if direction == "producer late" else STEPS
    plain_ms = sum(enqueue_ms[:steps])
    holds = []

    def before(watch):
        held_stream = side if direction == "producer late" else data_stream
        holds.append(watch.add(sh.hold(held_stream, sh.hold_length(plain_ms), direction)))

    got, got_probe, held_ms, watch = _run_pipeline(_draw_pipeline, source, steps, stream=data_stream, sync_each=False,
                                                   watch_names=("blur_fused", "mt19937_randn_device", "resample3d"), before=before)
    held = holds[0]
    draws = watch.of("mt19937_randn_device")
    assert len(draws) == steps and all(call[1] == side.stream_id for call in draws), draws  # the draws are made, on the draw stream
    consumers = watch.of("blur_fused", data_stream)
    assert len(consumers) == len(watch.of("blur_fused")) == steps
    # Only the launches in front of the first back-pressure wait of the HOST can be asked to have been enqueued under the hold:
    # with the data stream held such a wait ends with the hold.  The fifth call of `on_draw_stream` waits for the mark of the
    # first (`_DRAWS_IN_FLIGHT`).  Under "gated" the draw stream itself stands behind the held data stream (its gate is the
    # data stream's latest resampling launch), the plans it uploads stay queued, and the plan ring's three pinned buffers run
    # out one step sooner: the fourth step's `prefetch_plan` waits for the first plan's upload.
    before_host_waits = min(streams._DRAWS_IN_FLIGHT, noise_stream._PLAN_RING.length) if policy == "gated" else streams._DRAWS_IN_FLIGHT
    in_force = _assert_in_force(consumers[:before_host_waits], held, f"draw stream, {policy}, {direction}")
    _row(f"(b) draw stream, {policy}", direction, plain_ms, held, data_stream, in_force, held_ms)
    _assert_same_steps(got, expected, f"draw stream, {policy}, {direction}")
    if steps == STEPS:
        assert torch.equal(got_probe, probe)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the pinned rings
# ---------------------------------------------------------------------------------------------------------------------
def _torch_draws(seed, counts):
    generator = torch.Generator().manual_seed(seed)
    return [torch.randn(count, generator=generator) for count in counts]


def _assert_draws(got, seed, counts, what) -> None:
    for index, (expected, result) in enumerate(zip(_torch_draws(seed, counts), got, strict=True)):
        assert torch.equal(expected.view(torch.int32), result.cpu().view(torch.int32)), f"{what}: draw {index} of seed {seed} is not torch.randn's"


def _timed_enqueue(enqueue) -> float:
    clock = sh.Stopwatch()
    clock.start()
    enqueue()
    clock.stop()
    torch.cuda.synchronize()
    return clock.ms


def test_staging_ring_waits_for_the_upload_that_still_reads_a_buffer(hip, monkeypatch):
    """(c) The host road (`TIO_DEVICE_RNG=0`): draws are written into a pinned buffer of the staging ring (two per size) and
    uploaded `non_blocking`.  Four equal draws back to back on a HELD stream: the first two uploads are still queued when the
    third draw needs a buffer, so it has to wait for the first upload's event — writing sooner would send the third draw's
    values up as the first's.  Expected: `torch.randn` from a generator of the same seed."""
    monkeypatch.setenv("TIO_DEVICE_RNG", "0")
    count, seed = 1 << 18, 71
    assert noise_stream._STAGING_RING.length == 2
    stream = torch.cuda.Stream()

    def four_draws(normal):
        return [normal.randn((count,), "cuda") for _ in range(4)]

    with torch.cuda.stream(stream):
        plain_ms = _timed_enqueue(lambda: four_draws(ops.HostNormalStream(seed)))
        held = sh.hold(stream, sh.hold_length(plain_ms), "staging")
        normal = ops.HostNormalStream(seed)
        first_two = [normal.randn((count,), "cuda") for _ in range(2)]
        in_force = held.in_force()  # (the third draw waits on the host until the first upload is through: until the hold has ended)
        rest = [normal.randn((count,), "cuda") for _ in range(2)]
    torch.cuda.synchronize()
    assert in_force, f"the first two draws were enqueued after the hold of {held.ms:.0f} ms had ended"
    _row("(c) staging ring, four draws", "consumer late", plain_ms, held, stream, "2 of 2")
    _assert_draws(first_two + rest, seed, [count] * 4, "staging ring")


def test_staging_ring_serves_two_streams_drawing_alternately(hip, monkeypatch):
    """(c) One thread, two streams, one ring: a held stream and a free one draw alternately.  A buffer whose upload is queued
    behind the hold must not be handed to the free stream's draw (its event is recorded on the stream that issued the copy)."""
    monkeypatch.setenv("TIO_DEVICE_RNG", "0")
    count, seeds = 1 << 18, (72, 73)
    device = torch.device("cuda", torch.cuda.current_device())
    held_stream = torch.cuda.Stream()
    free_stream = sh.independent_stream(held_stream, device)

    def alternate(normals, on_first=None):
        drawn = ([], [])
        for index in range(4):
            for which, stream in enumerate((held_stream, free_stream)):
                with torch.cuda.stream(stream):
                    drawn[which].append(normals[which].randn((count,), "cuda"))
            if index == 0 and on_first is not None:
                on_first()
        return drawn

    plain_ms = _timed_enqueue(lambda: alternate([ops.HostNormalStream(seed) for seed in seeds]))
    # (In a run of the whole suite the host once stalled for longer than the 20 ms hold inside the first pair of draws (cause
    # not found: it did not happen when the file ran alone), and such a run says nothing about ordering either way.  The values of EVERY attempt are held to
    # torch.randn's; an attempt whose first pair missed its hold is made again, three at the most, and the last one must
    # have been enqueued under its hold.)
    for attempt in range(3):
        held = sh.hold(held_stream, sh.hold_length(plain_ms), "two streams")
        flags = []
        drawn = alternate([ops.HostNormalStream(seed) for seed in seeds], on_first=lambda: flags.append(held.in_force()))
        torch.cuda.synchronize()
        for which, seed in enumerate(seeds):
            _assert_draws(drawn[which], seed, [count] * 4, "two streams")
        if flags == [True]:
            break
    assert flags == [True], f"the first pair of draws was enqueued after the hold of {held.ms:.0f} ms had ended, three times"
    _row("(c) staging ring, two streams", "one stream held", plain_ms, held, free_stream, f"1 of 1 (attempt {attempt + 1})")


def test_plan_started_ahead_and_collected_late_keeps_its_pinned_buffer(hip, modes):
    """(c) `prefetch_plan` lends a pinned buffer of the plan ring (three per size) to a native job.  While it is lent — no
    upload event guards it — three more streams of the same size make and upload their plans on a HELD stream, which takes
    every other buffer of the ring and then waits for one; the plan started first is collected last.  Every stream's draws
    are `torch.randn`'s."""
    ops.set_noise_plan("host")  # (the device's plan starts nothing ahead for whole groups of 16)
    count, seeds = ops.HostNormalStream.DEVICE_DRAW_MIN, (81, 82, 83, 84)
    ring = noise_stream._PLAN_RING
    device_index = torch.cuda.current_device()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        plain_ms = _timed_enqueue(lambda: [ops.HostNormalStream(seed).randn((count,), "cuda") for seed in seeds])
        early = ops.HostNormalStream(seeds[0])
        early.prefetch_plan(count, "cuda")
        assert early._prefetched is not None and sum(buffer.lent for buffer in ring.buffers(device_index)) == 1
        held = sh.hold(stream, sh.hold_length(plain_ms), "plan ring")
        others = [ops.HostNormalStream(seed).randn((count,), "cuda") for seed in seeds[1:3]]
        in_force = held.in_force()
        others.append(ops.HostNormalStream(seeds[3]).randn((count,), "cuda"))  # (the ring is full: waits for an upload behind the hold)
        late = early.randn((count,), "cuda")
    torch.cuda.synchronize()
    assert in_force, f"the plans were uploaded after the hold of {held.ms:.0f} ms had ended"
    assert not any(buffer.lent for buffer in ring.buffers(device_index))
    _row("(c) plan ring, plan started ahead", "consumer late", plain_ms, held, stream, "2 of 2")
    for seed, drawn in zip(seeds, [late] + others, strict=True):
        _assert_draws([drawn], seed, [count], "plan ring")


# ---------------------------------------------------------------------------------------------------------------------
# (d) two data streams, one thread: the per-stream workspaces inside libtio_hip.so
# ---------------------------------------------------------------------------------------------------------------------
def _rotation_mappings(degrees_per_element, size):
    import numpy as np

    from torchio_amd.transforms import spatial as sp

    rows = []
    centre = (size - 1) / 2.0
    for degrees in degrees_per_element:
        rotation = sp._euler_to_rotation_matrix(np.asarray((degrees,) * 3, dtype=np.float64))
        shift = centre - rotation @ np.full(3, centre) + 1.5
        rows.append(np.concatenate([rotation, shift[:, None]], axis=1))
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def _workspace_jobs(hip):
    """The launches that use a per-stream workspace, each as (name, switches, two variants of `call() -> tensors`) — one
    variant per stream, with its own geometry: a workspace shared between the streams would mix them up."""
    geometry = dict(in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True, interps=["linear"])
    g = torch.Generator(device="cuda").manual_seed(41)
    large = torch.rand(3, 1, 256, 256, 256, generator=g, device="cuda") - 0.25  # 12 288 bricks: the smallest launch that folds its minimum
    small = torch.rand(2, 1, 96, 96, 96, generator=g, device="cuda")
    reduced = [torch.rand(2, 3, 40, 40, 40, generator=g, device="cuda") - 0.5 for _ in range(2)]
    half = torch.tensor([0.5], device="cuda")

    def folded_fast(variant):
        kwargs = dict(out_shape=(256,) * 3, mapping=_mapping(3, 43 + variant, scale=0.05, shift=3.0).cuda(), control_points=None,
                      fills=[torch.tensor([-0.5], device="cuda")], precision="fast", **geometry)
        assert starts_from_a_plan(hip, [large], **kwargs)

        def call():
            ops.expect_minimum_fill(True)  # (what a Compose announces for the child after this one)
            try:
                out = hip.resample3d([large], **kwargs)[0]
            finally:
                ops.expect_minimum_fill(False)
            folded = ops.folded_channel_min(out)
            assert folded is not None  # the launch folded the minimum: the keys of the stream's workspace were used
            return [out, folded]

        return call

    def plain_minimum(variant):
        return lambda: [hip.channel_min(reduced[variant])]

    def planned_exact_affine(variant):
        kwargs = dict(out_shape=(96,) * 3, mapping=_mapping(2, 51 + variant, scale=0.1, shift=4.0).cuda(), control_points=None, fills=[half],
                      precision="exact", **geometry)
        assert starts_from_a_plan(hip, [small], **kwargs)
        return lambda: [hip.resample3d([small], **kwargs)[0]]

    def lean_exact_listed(variant):
        # one element whose boxes exceed the staging tile (30 degrees about every axis) beside one whose boxes fit: with the hint,
        # the planner LISTS the first one's bricks behind the header of the plan — the 16 ints that must be zero between launches
        kwargs = dict(out_shape=(96,) * 3, mapping=_rotation_mappings([5, 30] if variant == 0 else [30, 7], 96).cuda(),
                      control_points=_control_points(2, (5, 5, 5), 61 + variant, amplitude=4.0).cuda(), fills=[half], precision="exact",
                      large_boxes=1, **geometry)
        assert starts_from_a_plan(hip, [small], **kwargs)
        return lambda: [hip.resample3d([small], **kwargs)[0]]

    return [
        ("planned FAST with the folded minimum", {"TIO_FAST_KERNEL": "planned"}, folded_fast),
        ("channel_min", {}, plain_minimum),
        ("planned exact affine", {"TIO_EXACT_PLAN": "2", "TIO_EXACT_LEAN": "0"}, planned_exact_affine),
        ("lean exact, multi-pass list", {"TIO_EXACT_LEAN": "2"}, lean_exact_listed),
    ]


def test_two_data_streams_keep_their_workspaces_apart(hip, modes, monkeypatch):
    """(d) One thread, two data streams — one held, one free —, launches enqueued alternately: the leased brick plan and its
    list header, the keys of the folded minimum and of `channel_min` are per stream.  Every result equals the same call
    issued alone."""
    device = torch.device("cuda", torch.cuda.current_device())
    held_stream = torch.cuda.Stream()
    free_stream = sh.independent_stream(held_stream, device)
    pair = (held_stream, free_stream)
    jobs = []
    for name, switches, make in _workspace_jobs(hip):
        for key, value in switches.items():
            monkeypatch.setenv(key, value)
        jobs.append((name, switches, [make(0), make(1)]))
        for key in switches:
            monkeypatch.delenv(key)
    torch.cuda.synchronize()

    def run_all(streams_of_variants):
        results = []
        for name, switches, calls in jobs:
            for key, value in switches.items():
                monkeypatch.setenv(key, value)
            per_variant = []
            for variant, stream in enumerate(streams_of_variants):
                with torch.cuda.stream(stream):
                    per_variant.append(calls[variant]())
            results.append(per_variant)
            for key in switches:
                monkeypatch.delenv(key)
        return results

    default = torch.cuda.current_stream()
    alone = run_all((default, default))
    torch.cuda.synchronize()
    # once on each stream without a hold: a stream's first launch sets its workspaces up and synchronises the device for it
    # (`min_workspace`), which under a hold would only wait for the hold to end
    clock = sh.Stopwatch()
    clock.start()
    warm = run_all(pair)
    clock.stop()
    torch.cuda.synchronize()
    with sh.watch(hip, ("resample3d", "channel_min")) as watch:
        held = watch.add(sh.hold(held_stream, sh.hold_length(clock.ms), "workspaces"))
        interleaved = run_all(pair)
    torch.cuda.synchronize()
    in_force = _assert_in_force(watch.calls, held, "two data streams")
    assert sorted({call[1] for call in watch.calls}) == sorted(stream.stream_id for stream in pair)
    _row("(d) two data streams", "one stream held", clock.ms, held, free_stream, in_force)
    for (name, _, _), expected, first, second in zip(jobs, alone, warm, interleaved, strict=True):
        for variant in range(2):
            for e, w, i in zip(expected[variant], first[variant], second[variant], strict=True):
                assert torch.equal(e, w), f"{name}: the first launch on stream {variant} differs from the call issued alone"
                assert torch.equal(e, i), f"{name}: the launch on stream {variant} ({'held' if variant == 0 else 'free'}) differs from the call issued alone"
    folded_out, folded = alone[0][0]
    assert torch.equal(folded.cpu(), folded_out[0].amin(dim=(1, 2, 3)).cpu())


def test_plan_workspace_grows_behind_a_held_stream(hip, monkeypatch):
    """(d) The growth path of the leased plan buffer: a 48^3 launch, then a 96^3 launch on the same HELD stream.  The second
    needs a larger buffer while the first one's plan is still unread behind the hold: `plan_workspace` has to wait for the
    stream before it frees (seen here as the host coming back only once the hold is over).  A free stream launches in between."""
    monkeypatch.setenv("TIO_FAST_KERNEL", "planned")
    device = torch.device("cuda", torch.cuda.current_device())
    # a stream of the high-priority pool: nothing else in the suite takes streams from it, so its plan buffer starts empty
    held_stream = torch.cuda.Stream(priority=-1)
    free_stream = sh.independent_stream(held_stream, device)
    g = torch.Generator(device="cuda").manual_seed(47)
    geometry = dict(in_spacing=(1, 1, 1), out_spacing=(1, 1, 1), affine_first=True, interps=["linear"], precision="fast", control_points=None)
    cases = []
    for index, size in enumerate((48, 96, 48)):
        data = torch.rand(2, 1, size, size, size, generator=g, device="cuda")
        kwargs = dict(out_shape=(size,) * 3, mapping=_mapping(2, 90 + index, scale=0.1, shift=3.0).cuda(), fills=[torch.tensor([0.25], device="cuda")], **geometry)
        assert starts_from_a_plan(hip, [data], **kwargs)
        cases.append((data, kwargs))
    alone = [hip.resample3d([data], **kwargs)[0] for data, kwargs in cases]
    torch.cuda.synchronize()
    held = sh.hold(held_stream, 50.0, "growth")
    with torch.cuda.stream(held_stream):
        small = hip.resample3d([cases[0][0]], **cases[0][1])[0]
    held_after_small = held.in_force()
    with torch.cuda.stream(free_stream):
        between = hip.resample3d([cases[2][0]], **cases[2][1])[0]
    with torch.cuda.stream(held_stream):
        grown = hip.resample3d([cases[1][0]], **cases[1][1])[0]
    held_after_grown = held.in_force()
    torch.cuda.synchronize()
    assert held_after_small, "the first launch was enqueued after the hold of 50 ms had ended"
    assert not held_after_grown, "the larger launch came back under the hold: the plan buffer of this stream did not have to grow"
    _row("(d) plan workspace growth", "consumer late", 0.0, held, free_stream, "1 of 1 (the growth waits for the stream)")
    assert torch.equal(small, alone[0]) and torch.equal(grown, alone[1]) and torch.equal(between, alone[2])


# ---------------------------------------------------------------------------------------------------------------------
# (e) two threads, one held stream
# ---------------------------------------------------------------------------------------------------------------------
def test_two_host_threads_enqueue_on_a_held_stream(hip, monkeypatch):
    """(e) The jobs of `test_two_host_threads_share_a_stream_without_sharing_a_plan`, three rounds, with the shared stream
    HELD so that both threads have enqueued everything before the first kernel runs: the pairs planner + sampler of the two
    threads then sit in the queue as the lease ordered them, and every result equals the call issued alone."""
    data, jobs = two_thread_jobs(hip, monkeypatch)
    stream = torch.cuda.Stream()
    orders = ([0, 1, 2, 3, 4, 5, 6, 7], [5, 2, 7, 0, 3, 6, 1, 4])
    rounds = 3
    with torch.cuda.stream(stream):
        clock = sh.Stopwatch()
        clock.start()
        serial = [hip.resample3d([data], precision=p, **kw)[0] for kw, p in jobs]
        clock.stop()
    torch.cuda.synchronize()
    plain_ms = clock.ms * rounds  # (each thread enqueues `rounds` times the eight jobs, beside the other)
    results: dict = {}
    flags: dict = {}
    errors: list = []
    held = sh.hold(stream, sh.hold_length(plain_ms), "two threads")

    def worker(which):
        try:
            with torch.cuda.stream(stream):  # the same stream in both threads
                outs = []
                for _ in range(rounds):
                    for n in orders[which]:
                        kw, p = jobs[n]
                        outs.append((n, hip.resample3d([data], precision=p, **kw)[0]))
                flags[which] = held.in_force()
                results[which] = outs
        except Exception as error:  # noqa: BLE001 - reported by the main thread
            errors.append(error)

    threads = [threading.Thread(target=worker, args=(which,)) for which in (0, 1)]
    for thread in threads:
        thread.start()
    for thread in threads:
        thread.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert flags == {0: True, 1: True}, f"a thread was still enqueueing when the hold of {held.ms:.0f} ms ended: {flags}"
    _row("(e) two threads, one stream", "consumer late", plain_ms, held, stream, "2 of 2 threads")
    for which in (0, 1):
        for n, out in results[which]:
            assert torch.equal(out, serial[n]), f"thread {which}: job {n} ({jobs[n][1]}) differs from its serial result"


# ---------------------------------------------------------------------------------------------------------------------
# (f) the caller's protocol for a plan made ahead
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fast", "exact"])
def test_callers_protocol_for_a_plan_made_ahead(hip, monkeypatch, precision):
    """(f) What `resample_plan` asks of its caller: the plan is made on one stream (held here: it is written late), the
    consuming stream waits for the maker's event and `record_stream`s the tensor, and then any number of calls may use it —
    three here, each with its own images.  2 x 96^3, elastic, forced onto the planned road."""
    monkeypatch.setenv(*AHEAD_ROADS[precision])
    device = torch.device("cuda", torch.cuda.current_device())
    maker = torch.cuda.Stream()
    consumer = sh.independent_stream(maker, device)
    batch, shape = 2, (96, 96, 96)
    g = torch.Generator(device="cuda").manual_seed(53)
    images = [torch.rand(batch, 1, *shape, generator=g, device="cuda") for _ in range(3)]
    geometry = dict(out_shape=shape, mapping=_mapping(batch, 57, scale=0.1, shift=4.0).cuda(),
                    control_points=_control_points(batch, (5, 5, 5), 58, amplitude=4.0).cuda(), in_spacing=(1, 1, 1), out_spacing=(1, 1, 1),
                    affine_first=True)
    launch = dict(interps=["linear"], fills=[torch.tensor([0.5], device="cuda")], precision=precision, **geometry)
    clock = sh.Stopwatch()
    clock.start()
    plain = [hip.resample3d([image], **launch)[0] for image in images]
    clock.stop()
    torch.cuda.synchronize()
    with sh.watch(hip, ("resample3d", "resample3d_plan")) as watch:
        held = watch.add(sh.hold(maker, sh.hold_length(clock.ms), "plan made ahead"))
        with torch.cuda.stream(maker):
            plan = hip.resample_plan(batch=batch, in_shape=shape, precision=precision, **geometry)
            ready = maker.record_event()
        assert plan is not None
        with torch.cuda.stream(consumer):
            consumer.wait_event(ready)
            plan.record_stream(consumer)
            ahead = [hip.resample3d([image], plan=plan, **launch)[0] for image in images]
    torch.cuda.synchronize()
    assert watch.names() == ["resample3d_plan"] + ["resample3d"] * 3
    in_force = _assert_in_force(watch.of("resample3d", consumer), held, f"plan made ahead, {precision}")
    _row(f"(f) caller's protocol, {precision}", "producer late", clock.ms, held, consumer, in_force)
    for index, (a, b) in enumerate(zip(plain, ahead, strict=True)):
        assert torch.equal(a, b), f"call {index} with the plan made ahead differs from the call that plans for itself"
