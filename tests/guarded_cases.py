"""The guarded cases: every engine entry point in guard-banded and misaligned buffers (``guarded_memory.py``).

One table for the CPU module (``test_guarded_memory.py``, the oracle engine) and the GPU module
(``test_gpu_guarded_memory.py``, the HIP engine).  A case records the engine method and its arguments, the inputs to carve
and which of them are shifted by one element at skew 1, the comparison bar (the one of the op's existing parity test — no
new ones), the ``TIO_*`` switches to set and the regions that must stay unwritten.  ``run_case`` carves every input, runs
the call with the engine's own allocations carved as well, then checks the guards, that every output element was written,
and the values.

What is shifted at skew 1: the volumes and the explicit noise draws — what a caller's dense view such as ``data[1:]`` hands
over.  Parameter tensors (taps, mappings, control points, fills, flags, tables) are carved between guards but keep their
alignment: the transforms upload them packed on 256-byte boundaries (``ops.h2d_packed``).  Shapes are the smallest that
still reach each road; the inputs keep the canary from being a legitimate result (finite floats, labels >= 0 and < 255,
fill values neither -1 nor 255).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass
from typing import Callable

import torch

import adjoint_reference as ar
from case_inputs import _blocky_labels
from case_inputs import _control_points
from case_inputs import _data
from case_inputs import _mapping
from case_inputs import _rotation_mapping
from case_inputs import _segments
from case_inputs import _taps
from guarded_memory import Arena
from guarded_memory import assert_untouched
from guarded_memory import assert_written
from guarded_memory import carve_like
from guarded_memory import guarded_engine_allocations

F32, F64, F16, BF16 = torch.float32, torch.float64, torch.float16, torch.bfloat16
U8, I8, I16, I32, I64 = torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64


# ---------------------------------------------------------------------------------------------------------------------
# bars: (want, got, what) -> None, every one taken from the existing test of its op
# ---------------------------------------------------------------------------------------------------------------------
def exact(want, got, what):
    """Bit for bit (``torch.equal``, as the parity tests)."""
    assert want.dtype == got.dtype and want.shape == got.shape, (what, want.dtype, got.dtype, want.shape, got.shape)
    assert torch.equal(want, got), f"{what}: {int((want != got).sum())} of {want.numel()} elements differ"


exact.is_exact = True


def close(rtol, atol):
    def bar(want, got, what):
        torch.testing.assert_close(got, want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")

    return bar


def absmax(bound):
    def bar(want, got, what):
        worst = float((want.double() - got.double()).abs().max()) if want.numel() else 0.0
        assert worst <= bound, f"{what}: max |difference| {worst:.3g} > {bound:.3g}"

    return bar


def of_scale(factor):
    """``max |d| <= factor * max |want|`` (the fast stencil against the exact one; the stencil's adjoint against the oracle's)."""

    def bar(want, got, what):
        scale = max(float(want.abs().max()), 1e-6)
        worst = float((want.double() - got.double()).abs().max())
        assert worst <= factor * scale, f"{what}: max |difference| {worst:.3g} > {factor:.3g} x {scale:.3g}"

    return bar


def per_voxel_1e4(want, got, what):
    """The bar of ``precision="tight"`` (test_gpu_tight.py): ``|d| <= 1e-4 max(|ref|, 1e-3 range)`` at every voxel."""
    want, got = want.double(), got.double()
    value_range = float(want.max() - want.min())
    rel = (want - got).abs() / want.abs().clamp_min(1e-3 * value_range)
    assert int((rel > 1e-4).sum()) == 0, f"{what}: {int((rel > 1e-4).sum())} voxels beyond 1e-4, worst {float(rel.max()):.3g}"


def rel_1e4(want, got, what):
    """The bar of ``precision="fast"`` (test_gpu_resample_planned.py): ``|d| / max(|ref|, 1) <= 1e-4``."""
    rel = (want.double() - got.double()).abs() / want.double().abs().clamp_min(1.0)
    assert int((rel > 1e-4).sum()) == 0, f"{what}: {int((rel > 1e-4).sum())} voxels beyond 1e-4, worst {float(rel.max()):.3g}"


# ---------------------------------------------------------------------------------------------------------------------
# the case record and its runner
# ---------------------------------------------------------------------------------------------------------------------
def _flatten(result, placed) -> list:
    if result is None:
        return []
    if isinstance(result, torch.Tensor):
        return [result]
    return [t for t in result if t is not None]


@dataclass(frozen=True)
class Case:
    id: str
    method: str                                   # the ``Engine`` method ...
    inputs: Callable[[], dict]                    # ... its tensors by name (CPU; a value may be a list, ``None`` entries allowed) ...
    arguments: Callable[[dict], tuple]            # ... and ``(args, kwargs)`` made of them
    skewed: tuple = ("data",)                     # the inputs that start one element off at skew 1 (every input is carved)
    bar: Callable = exact
    env: tuple = ()                               # ((name, value), ...) TIO_* switches
    stencil_precision: str | None = None
    call: Callable | None = None                  # (engine, placed) -> result, where the call is more than one method
    outputs: Callable = _flatten                  # (result, placed) -> the output tensors (caller-owned accumulators included)
    compared: Callable | None = None              # outputs -> the views that must be written and are compared (default: all)
    untouched: Callable | None = None             # outputs -> the views that must still be entirely canary
    reference: Callable | None = None             # (oracle, cpu inputs, hip or None) -> the expected outputs (default: the oracle's call)
    at_skew1: str = "same"                        # "none": the entry point's contract demands alignment, the call answers None
    skew_bits: bool | None = None                 # HIP at skew 1 == HIP at skew 0 bit for bit (default: wherever the bar is exact)
    proves: Callable | None = None                # (hip, placed) at skew 0 on the GPU: the road the case names was taken
    also: Callable | None = None                  # (compared outputs on the CPU, cpu inputs): what else the op's own test asserts
    engines: tuple = ("oracle", "hip")
    owned: bool = True                            # every returned output lies in the arena (the shim caught its allocation)

    @property
    def bits_at_skew(self) -> bool:
        return getattr(self.bar, "is_exact", False) if self.skew_bits is None else self.skew_bits


def _place(value, place):
    if isinstance(value, torch.Tensor):
        return place(value)
    if isinstance(value, (list, tuple)):
        return type(value)(_place(v, place) for v in value)
    return value


def _invoke(case: Case, engine, placed):
    if case.call is not None:
        return case.call(engine, placed)
    args, kwargs = case.arguments(placed)
    return getattr(engine, case.method)(*args, **kwargs)


@contextlib.contextmanager
def _stencil_precision(mode):
    import torchio_amd as tio

    previous = tio.get_stencil_precision()
    if mode is not None:
        tio.set_stencil_precision(mode)
    try:
        yield
    finally:
        tio.set_stencil_precision(previous)


_REFERENCES: dict = {}  # (case id, reference engine) -> expected outputs on the CPU: computed once, shared, never changed


def expected_outputs(case: Case, oracle, hip=None) -> list:
    key = (case.id, "hip" if hip is not None and case.reference is not None else "oracle")
    if key not in _REFERENCES:
        cpu = case.inputs()  # (fresh tensors: the in-place ops write into their own copies)
        if case.reference is not None:
            outs = case.reference(oracle, cpu, hip)
        else:
            outs = case.outputs(_invoke(case, oracle, cpu), cpu)
        outs = [t.detach().cpu() for t in outs]
        _REFERENCES[key] = outs if case.compared is None else [t.clone() for t in case.compared(outs)]
    return _REFERENCES[key]


def run_case(case: Case, engine, device, skew: int, monkeypatch, oracle, hip=None) -> list | None:
    """One guarded call of *case* on *engine*; returns the compared outputs on the CPU (``None`` where the contract says the
    call answers ``None``).  Order: guards, then unwritten elements, then values."""
    for name, value in case.env:
        monkeypatch.setenv(name, value)
    cpu = case.inputs()
    arena = Arena()
    placed = {
        name: _place(value, lambda t, name=name: carve_like(t, arena, device, skew if name in case.skewed else 0, label=f"{case.id}:{name}"))
        for name, value in cpu.items()
    }
    if skew == 0 and case.proves is not None and engine.name == "hip":
        case.proves(engine, placed)
    with _stencil_precision(case.stencil_precision), guarded_engine_allocations(arena):
        result = _invoke(case, engine, placed)
        if engine.device_type == "cuda":
            torch.cuda.synchronize()
    arena.check_guards()
    if skew == 1 and case.at_skew1 == "none" and engine.name == "hip":
        assert result is None, f"{case.id}: a misaligned pointer must be refused (the contract demands 16 bytes)"
        return None
    outs = case.outputs(result, placed)
    assert outs, f"{case.id}: the call returned nothing"
    if case.owned:
        for n, out in enumerate(_flatten(result, placed)):
            assert arena.owns(out), f"{case.id}: output {n} was not allocated through the guarded shim"
    for n, view in enumerate(case.untouched(outs) if case.untouched is not None else []):
        assert_untouched(view, f"{case.id}: region {n} the call promises to leave alone")
    views = outs if case.compared is None else case.compared(outs)
    for n, view in enumerate(views):
        assert_written(view, f"{case.id}: output {n}")
    got = [view.detach().cpu() for view in views]
    for n, (want, have) in enumerate(zip(expected_outputs(case, oracle, hip), got, strict=True)):
        case.bar(want, have, f"{case.id}: output {n} at skew {skew}")
    if case.also is not None:
        case.also(got, cpu)
    return got


CASES: list[Case] = []


def _add(**fields) -> None:
    CASES.append(Case(**fields))


# ---------------------------------------------------------------------------------------------------------------------
# stencil
# ---------------------------------------------------------------------------------------------------------------------
def _conv_inputs(shape, dtype, seed, sigmas, stride, skip=None):
    def build():
        taps, _ = _taps(len(sigmas), sigmas, stride)
        t = {"data": _data(shape, dtype, seed), "taps": taps}
        if skip is not None:
            t["skip"] = torch.tensor(skip, dtype=U8)
        return t

    return build


def _conv_arguments(sigmas, stride):
    radius = _taps(len(sigmas), sigmas, stride)[1]
    return lambda t: ((t["data"], t["taps"], radius), {"skip": t.get("skip")})


def _stencil_adjoint_bar(radius):
    return of_scale(2e-6 * (2 * max(radius) + 1))  # test_stencil_adjoint.py: 2e-6 of max |expected| per tap of the longest axis


def _add_conv(name, shape, dtype=F32, sigmas=((1.3, 0.6, 2.0),), stride=32, skip=None, env=(), adjoint=True, also=None, seed=16):
    common = dict(inputs=_conv_inputs(shape, dtype, seed, list(sigmas), stride, skip), arguments=_conv_arguments(list(sigmas), stride), env=env)
    _add(id=f"conv-{name}", method="separable_conv3d", also=also, **common)
    if adjoint:  # (float32 whatever comes in: the gradient's type)
        radius = _taps(len(sigmas), list(sigmas), stride)[1]
        _add(id=f"conv_adjoint-{name}", method="separable_conv3d_adjoint", bar=_stencil_adjoint_bar(radius), skew_bits=True, **common)


for _dtype, _name in ((F32, "f32"), (F16, "f16"), (BF16, "bf16"), (F64, "f64")):
    _add_conv(f"generic-{_name}", (2, 2, 19, 23, 70), _dtype, adjoint=_dtype == F32)
_add_conv("marching_segments", (1, 1, 70, 40, 64), seed=61)
_add_conv("several_k_tiles", (1, 1, 9, 50, 520), seed=61)
_add_conv("k256", (1, 2, 37, 5, 256), seed=61)
_add_conv("k4", (2, 1, 9, 33, 4), seed=61)
for _sigmas in ((0.5, 0.5, 3.5), (3.1, 4.0, 0.4), (0.5, 0.5, 6.0), (5.5, 0.3, 2.7)):
    _add_conv("radius_class-" + "_".join(str(s) for s in _sigmas), (1, 1, 45, 41, 128), sigmas=(_sigmas,), stride=48, seed=63, adjoint=False)


def _skipped_row_is_the_input(got, cpu):
    assert torch.equal(got[0][1], cpu["data"][1]), "the skipped element's output must equal its input"


_add_conv("per_element_skip", (3, 1, 12, 14, 66), sigmas=((1.0, 0.0, 0.7), (0.0, 0.0, 0.0), (0.4, 0.0, 1.9)), stride=16, skip=[0, 1, 0],
          seed=17, also=_skipped_row_is_the_input)
_add_conv("float4_per_element_skip", (3, 1, 40, 36, 128), sigmas=((1.0, 1.7, 0.7), (0.0, 0.0, 0.0), (0.4, 0.5, 1.9)), stride=16, skip=[0, 1, 0],
          seed=62, also=_skipped_row_is_the_input, adjoint=False)
_add_conv("ring", (1, 1, 70, 40, 64), env=(("TIO_CONV_RING", "1"),), seed=61, adjoint=False)
_add_conv("no_fuse", (1, 1, 70, 40, 64), env=(("TIO_CONV_NO_FUSE", "1"),), seed=61, adjoint=False)
_add(
    id="conv-one_voxel_axes", method="separable_conv3d",
    inputs=lambda: {"data": _data((2, 1, 1, 6, 4), F32, 83), "taps": torch.tensor([[0.25, 0.5, 0.25]]).repeat(3, 1)[None].contiguous()},
    arguments=lambda t: ((t["data"], t["taps"], [1, 1, 1]), {}),
)


# ---------------------------------------------------------------------------------------------------------------------
# fused stencil: Noise(Blur(BiasField(data))) in the stencil's passes.  The oracle has no fused form: there (and as the
# reference) the three ops run one after the other.  Alignment is part of the contract: at skew 1 the call answers None.
# ---------------------------------------------------------------------------------------------------------------------
_FUSED_SHAPE = (2, 1, 40, 36, 64)


def _fused_inputs(sigmas, bias, noise):
    def build():
        taps, _ = _taps(len(sigmas), list(sigmas), 32)
        t = {"data": _data(_FUSED_SHAPE, F32, 31), "taps": taps}
        if bias:
            t["coarse"] = 0.3 * torch.randn(2, 1, 4, 4, 4, generator=torch.Generator().manual_seed(32))
        if noise is not None:
            t["mean"], t["std"] = torch.zeros(2), torch.full((2,), 0.25)
        if noise == "draws":
            t["draws"] = torch.randn(_FUSED_SHAPE, generator=torch.Generator().manual_seed(33))
        return t

    return build


def _fused_call(sigmas, noise):
    radius = _taps(len(sigmas), list(sigmas), 32)[1]

    def separately(engine, t):
        out = t["data"] if "coarse" not in t else engine.bias_field_apply(t["data"], t["coarse"])
        out = engine.separable_conv3d(out, t["taps"], radius)
        if noise == "philox":
            out = engine.add_noise(out, t["mean"], t["std"], philox_seed=4321)
        elif noise == "draws":
            out = engine.add_noise(out, t["mean"], t["std"], base1=t["draws"])
        return out

    def call(engine, t):
        if engine.name != "hip":
            return separately(engine, t)
        how = None if noise is None else (t["mean"], t["std"], 4321 if noise == "philox" else t["draws"])
        return engine.blur_fused(t["data"], t["taps"], radius, bias_coarse=t.get("coarse"), noise=how)

    return call, separately


def _add_fused(name, sigmas=((1.6, 1.1, 1.9), (1.2, 1.9, 0.8)), bias=True, noise=None, precision="exact", env=()):
    call, separately = _fused_call(sigmas, noise)

    def reference(oracle, cpu, hip):
        if precision == "fast" and hip is not None:  # the fast taps against the exact launch, as test_gpu_lazy_fusion.py does
            with _stencil_precision("exact"):
                return [call(hip, {name: _place(value, lambda t: t.cuda()) for name, value in cpu.items()}).cpu()]
        return [separately(oracle, cpu)]

    _add(
        id=f"blur_fused-{name}", method="blur_fused", inputs=_fused_inputs(sigmas, bias, noise), arguments=lambda t: ((), {}), call=call,
        reference=reference, stencil_precision=precision, env=env, at_skew1="none", skewed=("draws",) if noise == "draws" else ("data",),
        # exact taps: bit for bit the unfused stencil (test_fused_jk_stage_every_k_radius) when nothing rides along; with the bias
        # field's exp / the Philox draws' log and cos the bar of test_lazy_fusion_matches_oracle_and_is_invisible
        bar=of_scale(2e-6) if precision == "fast" else (exact if not bias and noise is None else close(1e-5, 2e-5)), skew_bits=False,
    )


_add_fused("plain", bias=False)
_add_fused("bias")
_add_fused("bias_philox", noise="philox")
_add_fused("bias_draws", noise="draws")
_add_fused("bias_philox-fast", noise="philox", precision="fast")
_add_fused("bias_draws-ring", noise="draws", env=(("TIO_CONV_RING", "1"),))
_add_fused("bias_philox-ring", noise="philox", env=(("TIO_CONV_RING", "1"),))
_add_fused("bias-radius7", sigmas=((6.5 / 3, 1.1, 1.9),))  # beyond the bias variant's register window: the ring kernel's natural road
_add_fused("bias-radius8", sigmas=((7.5 / 3, 1.1, 1.9),))


# ---------------------------------------------------------------------------------------------------------------------
# pointwise
# ---------------------------------------------------------------------------------------------------------------------
def _third_row_is_the_input(got, cpu):
    assert torch.equal(got[0][2], cpu["data"][2])


for _divide in (False, True):
    _add(
        id=f"bias_field-{'divide' if _divide else 'multiply'}", method="bias_field_apply",
        inputs=lambda: {"data": _data((3, 2, 18, 21, 68), F32, 18), "coarse": 0.5 * torch.randn(3, 2, 4, 5, 6, generator=torch.Generator().manual_seed(19)),
                        "skip": torch.tensor([0, 0, 1], dtype=U8)},
        arguments=lambda t, divide=_divide: ((t["data"], t["coarse"]), {"divide": divide, "skip": t["skip"]}),
        bar=close(2e-6, 0), also=_third_row_is_the_input,
    )


def _gamma_inputs():
    data = _data((3, 2, 9, 11, 31), F32, 23)
    data[0, 0, 0, 0, :4] = torch.tensor([0.0, -0.0, 1.0, -1.0])
    return {"data": data, "gamma": torch.tensor([0.8, 1.0, 1.3])}


_add(id="gamma_pow", method="gamma_pow", inputs=_gamma_inputs, arguments=lambda t: ((t["data"], t["gamma"]), {}), bar=close(2e-6, 0))


def _noise_inputs(shape=(3, 2, 9, 11, 31), draws=2):
    def build():
        g = torch.Generator().manual_seed(21)
        t = {"data": _data(shape, F32, 20), "mean": torch.tensor([0.1, 0.0, -0.2]), "std": torch.tensor([0.25, 0.0, 0.5]),
             "keep": torch.tensor([1, 0, 1], dtype=U8)}
        for n in range(draws):
            t[f"base{n + 1}"] = torch.randn(shape, generator=g)
        return t

    return build


def _kept_row_is_the_input(got, cpu):
    assert torch.equal(got[0][1], cpu["data"][1])


_add(id="add_noise-draws", method="add_noise", inputs=_noise_inputs(draws=1), skewed=("data", "base1"), also=_kept_row_is_the_input,
     arguments=lambda t: ((t["data"], t["mean"], t["std"]), {"base1": t["base1"], "keep": t["keep"]}))
_add(id="add_noise-rician", method="add_noise", inputs=_noise_inputs(draws=2), skewed=("data", "base1", "base2"), bar=close(1e-6, 1e-7),
     also=_kept_row_is_the_input,
     arguments=lambda t: ((t["data"], t["mean"], t["std"]), {"rician": True, "base1": t["base1"], "base2": t["base2"], "keep": t["keep"]}))
for _shape, _name in (((2, 1, 8, 8, 64), "4n"), ((2, 1, 3, 5, 29), "4n+3")):  # (435 = 4 x 108 + 3 elements per row)
    _add(id=f"add_noise-philox-{_name}", method="add_noise", inputs=lambda shape=_shape: {"data": _data(shape, F32, 22)},
         arguments=lambda t: ((t["data"], 0.0, 0.25), {"philox_seed": 99}), bar=close(0, 1e-6))


def _philox_direct(engine, t):
    """``Engine.philox_normal`` never hands over a shifted output: the entry point itself, on the carved (shifted) buffer."""
    out = t["out"]
    engine._call("philox_normal", out, C.c_void_p(out.data_ptr()), out.numel(), 1234567890123, 0, engine._stream(out))
    return out


_add(id="philox_normal", method="philox_normal", inputs=lambda: {}, arguments=lambda t: (((4003,), 1234567890123, 0, _DEVICE[0]), {}),
     bar=close(4e-7, 1e-7), skew_bits=True, reference=lambda oracle, cpu, hip: [oracle.philox_normal((4003,), 1234567890123, 0, "cpu")])
_add(id="philox_normal-callers_buffer", method="philox_normal", inputs=lambda: {"out": torch.zeros(4003)}, skewed=("out",), arguments=lambda t: ((), {}),
     call=_philox_direct, outputs=lambda result, t: [t["out"]], owned=False, bar=close(4e-7, 1e-7), skew_bits=True,
     reference=lambda oracle, cpu, hip: [oracle.philox_normal((4003,), 1234567890123, 0, "cpu")])
_DEVICE = ["cpu"]  # where an op without tensor arguments makes its output: set by the test modules before a case runs

for _dtype, _name in ((F32, "f32"), (F16, "f16"), (I16, "i16"), (F64, "f64")):
    _add(id=f"channel_min-{_name}", method="channel_min", inputs=lambda dtype=_dtype: {"data": _data((3, 4, 11, 13, 17), dtype, 15)},
         arguments=lambda t: ((t["data"],), {}))
_add(id="channel_min-float4", method="channel_min", inputs=lambda: {"data": _data((2, 3, 8, 9, 12), F32, 15)}, arguments=lambda t: ((t["data"],), {}))


# ---------------------------------------------------------------------------------------------------------------------
# the reference's noise stream (HostNormalStream: mt19937 + torch's Box-Muller), host road and device road
# ---------------------------------------------------------------------------------------------------------------------
def _stream_randn(count):
    def call(engine, t):
        from torchio_amd import ops

        return ops.HostNormalStream(2024).randn((count,), _DEVICE[0])

    return call


def _bits(want, got, what):
    assert torch.equal(want.view(torch.int32), got.view(torch.int32)), what  # (signed zeros included, as test_gpu_device_rng.py)


_bits.is_exact = True

for _count in (4003, 1 << 20, 1_500_003, (1 << 20) + 16 * 39 * 3 + 32):  # host road; whole groups; a partial group of 16; inside a state block
    _add(id=f"host_stream-randn-{_count}", method="HostNormalStream.randn", inputs=lambda: {}, arguments=lambda t: ((), {}), call=_stream_randn(_count),
         reference=lambda oracle, cpu, hip, count=_count: [torch.randn(count, generator=torch.Generator().manual_seed(2024))], bar=_bits,
         engines=("hip",) if _count > 4003 else ("oracle", "hip"))


def _stream_add_noise(engine, t):
    from torchio_amd import ops

    out = ops.HostNormalStream(2024).add_noise(t["data"], t.get("mean", 0.75), t.get("std", 1.5))
    assert out is not None, "the fused draw-and-sum launch did not take this form"
    return out


def _stream_add_noise_reference(oracle, cpu, hip):
    base = torch.randn(cpu["data"].shape, generator=torch.Generator().manual_seed(2024))
    return [oracle.add_noise(cpu["data"], cpu.get("mean", 0.75), cpu.get("std", 1.5), rician=False, base1=base)]


for _shape, _batched in (((2, 1, 96, 96, 96), False), ((3, 2, 64, 80, 71), True)):  # (the second: not a multiple of 16 — torch's tail rule)
    def _inputs(shape=_shape, batched=_batched):
        t = {"data": torch.rand(*shape, generator=torch.Generator().manual_seed(1)) * 100 - 20}
        if batched:
            t["mean"], t["std"] = torch.tensor([0.5, -1.25, 3.0]), torch.tensor([0.1, 2.0, 0.5])
        return t

    _add(id=f"host_stream-add_noise-{'x'.join(str(s) for s in _shape)}", method="HostNormalStream.add_noise", inputs=_inputs, arguments=lambda t: ((), {}),
         call=_stream_add_noise, reference=_stream_add_noise_reference, bar=_bits, engines=("hip",))


# ---------------------------------------------------------------------------------------------------------------------
# resampling
# ---------------------------------------------------------------------------------------------------------------------
def _resample(name, in_shape, out_shape=None, *, batch=2, images=((2, F32, "linear", True),), elastic=False, cp_shape=(7, 6, 5), env=(),
              precision=None, large_boxes=0, bar=exact, spacing=((1.0, 1.25, 0.8), (0.9, 1.1, 0.75)), affine_first=True, mapping=None,
              mapping_args=dict(scale=0.15, shift=3.0), passthrough=None, cp_skip=None, planned=False, labels=None, skew_bits=None, also=None,
              engines=("oracle", "hip"), amplitude=4.0, seed=1):
    """``images``: ``(channels, dtype, interpolation, with a fill rule)`` per image; ``labels``: label count of "label" images."""
    out_shape = tuple(out_shape or in_shape)
    interps = [image[2] for image in images]

    def inputs():
        t = {"data": [], "fills": []}
        for n, (channels, dtype, interp, with_fill) in enumerate(images):
            shape = (batch, channels, *in_shape)
            t["data"].append(_blocky_labels(shape, dtype, seed + n, labels) if interp == "label" else _data(shape, dtype, seed + n))
            # (fill values: neither -1 nor 255, and none of the labels 0..6)
            t["fills"].append(torch.tensor([9.0, 11.0, 13.0][:channels]) if with_fill and interp == "nearest"
                              else (torch.tensor([-1.5, 0.5, 0.25][:channels]) if with_fill and interp != "label" else None))
        t["mapping"] = mapping() if mapping is not None else _mapping(1, seed + 1, **mapping_args)
        if elastic:
            t["control_points"] = _control_points(1, cp_shape, seed + 2, amplitude)
        if passthrough is not None:
            t["passthrough"] = torch.tensor(passthrough, dtype=U8)
        if cp_skip is not None and elastic:
            t["cp_skip"] = torch.tensor(cp_skip, dtype=U8)
        if labels is not None:
            t["tables"] = [torch.unique(d).double() if i == "label" else None for d, i in zip(t["data"], interps)]
        return t

    def geometry(t):
        return dict(out_shape=out_shape, mapping=t["mapping"], control_points=t.get("control_points"), in_spacing=spacing[0],
                    out_spacing=spacing[1], affine_first=affine_first, cp_skip=t.get("cp_skip"), passthrough=t.get("passthrough"))

    def arguments(t, precision=precision):
        kwargs = dict(interps=interps, fills=t["fills"], precision=precision, large_boxes=large_boxes, **geometry(t))
        if labels is not None:
            kwargs.update(label_tables=t["tables"], pad_labels=[7.0] * len(images))
        return (t["data"],), kwargs

    def reference(oracle, cpu, hip):  # (the oracle computes the reference's own arithmetic: what every precision is held against)
        args, kwargs = arguments(cpu, precision="exact")
        return oracle.resample3d(*args, **kwargs)

    def proves(hip, t):
        plan = hip.resample_plan(batch=batch, in_shape=in_shape, precision=precision, large_boxes=large_boxes, **geometry(t))
        assert plan is not None, f"resample-{name}: this launch does not start from a brick plan, the planned road was not taken"

    _add(id=f"resample-{name}", method="resample3d", inputs=inputs, arguments=arguments, reference=reference, env=env, bar=bar,
         proves=proves if planned else None, skew_bits=skew_bits, also=also, engines=engines)


def _each_geometry(name, *args, **kwargs):
    """With and without a fill rule, affine and affine + elastic."""
    images = kwargs.pop("images", ((2, F32, "linear", None),))
    for elastic in (False, True):
        for fill in (False, True):
            these = tuple((c, d, i, fill if f is None else f) for c, d, i, f in images)
            _resample(f"{name}-{'elastic' if elastic else 'affine'}-{'fill' if fill else 'zero'}", *args, images=these, elastic=elastic, **kwargs)


_UNIT = ((1, 1, 1), (1, 1, 1))
_GATHER = (("TIO_RESAMPLE_PATH", "gather"),)
_LEAN = (("TIO_EXACT_LEAN", "2"), ("TIO_FAST_KERNEL", "planned"))
_each_geometry("gather", (18, 21, 37), env=_GATHER)
_resample("gather-f16", (18, 21, 37), images=((2, F16, "linear", True),), elastic=True, env=_GATHER)
_resample("gather-i16-nearest", (18, 21, 37), images=((2, I16, "nearest", True),), elastic=True, env=_GATHER)
_each_geometry("brick", (33, 40, 36), (35, 29, 50))  # no output extent a multiple of 16
_resample("planned_brick-zero", (40, 40, 37), env=(("TIO_EXACT_PLAN", "2"),), precision="exact", spacing=_UNIT, planned=True, batch=3,
          images=((1, F32, "linear", False), (1, I16, "nearest", False)), mapping_args=dict(scale=0.1, shift=3.0))
_resample("planned_brick-fill", (40, 40, 37), env=(("TIO_EXACT_PLAN", "2"),), precision="exact", spacing=_UNIT, planned=True, batch=3,
          images=((1, F32, "linear", True), (1, I16, "nearest", False)), mapping_args=dict(scale=0.4, shift=20.0))
_LEAN_COMMON = dict(env=_LEAN, spacing=_UNIT, planned=True, cp_shape=(3, 3, 3), mapping_args=dict(scale=0.1, shift=4.0), batch=3)
_each_geometry("lean_exact", (70, 52, 56), precision="exact", images=((1, F32, "linear", None),), **_LEAN_COMMON)
_each_geometry("lean_tight", (70, 52, 56), precision="tight", images=((1, F32, "linear", None),), bar=per_voxel_1e4, **_LEAN_COMMON)
_resample("lean_exact-two_channels", (70, 52, 56), precision="exact", images=((1, F32, "linear", True), (2, F32, "linear", True)), elastic=True,
          passthrough=[0, 0, 1], cp_skip=[0, 1, 0], **_LEAN_COMMON)
_resample("lean_tight-two_channels", (70, 52, 56), precision="tight", images=((1, F32, "linear", True), (2, F32, "linear", True)), elastic=True,
          passthrough=[0, 0, 1], cp_skip=[0, 1, 0], bar=per_voxel_1e4, **_LEAN_COMMON)
for _dtype, _size in ((U8, 1), (I16, 2), (I32, 4), (I64, 8)):
    _resample(f"lean_exact-label_map_of_{_size}_bytes", (70, 52, 56), precision="exact", elastic=_size in (2, 8),
              images=((1, F32, "linear", True), (1, _dtype, "nearest", False)), **_LEAN_COMMON)
_each_geometry("planned_fast", (64, 64, 64), precision="fast", env=(("TIO_FAST_KERNEL", "planned"),), bar=rel_1e4, spacing=_UNIT, planned=True,
               cp_shape=(3, 3, 3), mapping_args=dict(scale=0.1, shift=4.0), batch=3, images=((1, F32, "linear", None), (2, F32, "linear", None)))
for _level in (1, 2):  # boxes beyond the staging tile: listed and walked behind the main kernel (1), staged in passes by every block (2)
    _resample(f"large_boxes_hint_{_level}", (64, 64, 64), precision="exact", large_boxes=_level, env=_LEAN, spacing=_UNIT, planned=True,
              mapping=lambda: _rotation_mapping(45, 64), images=((1, F32, "linear", True),), batch=2)
    _resample(f"large_boxes_hint_{_level}-elastic", (64, 64, 64), precision="exact", large_boxes=_level, env=_LEAN, spacing=_UNIT, planned=True,
              mapping=lambda: _rotation_mapping(45, 64), images=((1, F32, "linear", False),), batch=2, elastic=True, cp_shape=(3, 3, 3))
for _dtype, _size in ((U8, 1), (I16, 2), (I32, 4), (I64, 8), (F32, "f32"), (F64, "f64")):
    for _fill in (False, True):
        _resample(f"nearest-{_size}-{'fill' if _fill else 'zero'}", (37, 41, 70), images=((2, _dtype, "nearest", _fill),), elastic=_fill,
                  cp_shape=(6, 5, 7), spacing=((1.0, 1.5, 0.8), (1.0, 1.5, 0.8)), mapping_args=dict(scale=0.12, shift=2.5), seed=3)
for _count in (4, 40):
    _resample(f"label_pv-{_count}_labels", (20, 18, 22), (19, 21, 20), images=((1, I16, "label", False),), labels=_count, spacing=_UNIT,
              mapping_args=dict(scale=0.2, shift=3.0), seed=11)
_resample("degenerate-1x9x1", (1, 9, 1), (3, 4, 2), images=((1, F32, "linear", True),), spacing=_UNIT, mapping_args=dict(scale=0.3, shift=0.4), seed=81)
_resample("degenerate-1x9x1-nearest", (1, 9, 1), (3, 4, 2), images=((1, I16, "nearest", True),), spacing=_UNIT, mapping_args=dict(scale=0.3, shift=0.4), seed=81)


def _passthrough_is_the_input(got, cpu):
    for out, data in zip(got, cpu["data"], strict=True):
        assert torch.equal(out[2], data[2]), "a passthrough element is a bit-exact copy of its input"


_resample("passthrough", (16, 20, 66), batch=4, images=((1, F32, "linear", True), (2, F32, "linear", True), (1, I16, "nearest", False)), elastic=True,
          cp_shape=(7, 7, 7), spacing=_UNIT, mapping_args=dict(scale=0.08, shift=3.0), cp_skip=[0, 1, 0, 0], passthrough=[0, 0, 1, 0], seed=7,
          also=_passthrough_is_the_input)

# B-spline order 3: the recursive prefilter, then sampling of the coefficients
for _shape in ((24, 20, 28), (5, 3, 2)):
    _add(id=f"bspline_prefilter-{'x'.join(str(s) for s in _shape)}", method="bspline_prefilter",
         inputs=lambda shape=_shape: {"data": torch.rand(2, 2, *shape, generator=torch.Generator().manual_seed(7)) * 40 - 10},
         arguments=lambda t: ((t["data"], 3), {}))
    _resample(f"cubic-{'x'.join(str(s) for s in _shape)}", _shape, images=((2, F32, "cubic", False),), elastic=_shape[0] > 5, cp_shape=(5, 6, 7),
              amplitude=3.0, spacing=((1.0, 1.5, 0.8), (1.1, 1.2, 0.9)), mapping_args=dict(scale=0.12, shift=3.0 if _shape[0] > 5 else 0.5), seed=8)


# the adjoint of the trilinear resampling: a scatter into a caller-owned, zeroed accumulator
_ADJOINT_SHAPE = (2, 3, 20, 18, 26)


def _adjoint_geometry(t=None):
    mapping = ar.scaled_mapping(_ADJOINT_SHAPE[2:], (22, 17, 25), zoom=0.9, shift=(0.7, -0.4, 1.1), skew=0.05)[None]
    return ar.geometry(in_shape=_ADJOINT_SHAPE[2:], out_shape=(22, 17, 25), mapping=mapping if t is None else t["mapping"],
                       control_points=None if t is None else t["control_points"])


def _adjoint_inputs():
    g = torch.Generator().manual_seed(23)
    return {"data": torch.zeros(_ADJOINT_SHAPE), "grad": torch.randn(2, 3, 22, 17, 25, generator=g), "mapping": _adjoint_geometry()["mapping"],
            "control_points": _control_points(1, (5, 5, 5), 24, amplitude=1.5), "fill": torch.linspace(0.4, -0.8, 3)}


def _adjoint_bar(want, got, what):  # test_gpu_adjoint.py: same weights and gates, another order of the additions
    cpu = _adjoint_inputs()
    ar.assert_within(got, want, ar.order_tolerance(_adjoint_geometry(cpu), cpu["grad"]), what)


_add(id="resample-linear_adjoint", method="resample3d", inputs=_adjoint_inputs, skewed=("data", "grad"), bar=_adjoint_bar, skew_bits=False,
     arguments=lambda t: (([t["data"]],), dict(interps=["linear_adjoint"], fills=[t["fill"]], _adjoint_of=[t["grad"]], **ar._launch_arguments(_adjoint_geometry(t)))),
     outputs=lambda result, t: [t["data"]], owned=False)


# the folded minimum: a lean launch of >= 12 288 bricks hands back the per-channel minimum of element 0 with its stores
def _folded_outputs(result, t):
    from torchio_amd import ops

    folded = ops.folded_channel_min(result[0])
    assert folded is not None and folded.shape == (1,), "the launch was not asked for the folded minimum"
    return [result[0], folded]


def _folded_is_the_reduction(got, cpu):
    assert torch.equal(got[1], got[0][0].amin(dim=(1, 2, 3)))


_add(id="resample-folded_minimum", method="resample3d", engines=("hip",), env=_LEAN + (("TIO_FOLDED_MIN", "1"),),
     inputs=lambda: {"data": [_data((1536, 1, 16, 16, 16), F32, 41)], "mapping": _mapping(1, 43, scale=0.05, shift=1.0), "fill": torch.tensor([-1.5])},
     arguments=lambda t: ((t["data"],), dict(out_shape=(17, 17, 17), mapping=t["mapping"], control_points=None, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1),
                                             affine_first=True, interps=["linear"], fills=[t["fill"]], precision="exact")),
     outputs=_folded_outputs, owned=False, also=_folded_is_the_reduction,
     reference=lambda oracle, cpu, hip: (lambda out: [out, out[0].amin(dim=(1, 2, 3))])(oracle.resample3d(
         cpu["data"], out_shape=(17, 17, 17), mapping=cpu["mapping"], control_points=None, in_spacing=(1, 1, 1), out_spacing=(1, 1, 1),
         affine_first=True, interps=["linear"], fills=[cpu["fill"]], precision="exact")[0]))


# ---------------------------------------------------------------------------------------------------------------------
# the data movers, F.interpolate's users, labels
# ---------------------------------------------------------------------------------------------------------------------
for _dtype, _mode, _out in ((F32, "linear", (20, 9, 7)), (F32, "linear", (5, 18, 33)), (F32, "nearest", (13, 9, 20)), (F32, "linear", (1, 1, 1)),
                            (F16, "linear", (5, 18, 33)), (I16, "nearest", (20, 9, 7)), (U8, "nearest", (5, 18, 33)), (I64, "linear", (20, 9, 7))):
    _add(id=f"interpolate3d-{str(_dtype).split('.')[-1]}-{_mode}-{'x'.join(str(s) for s in _out)}", method="interpolate3d",
         inputs=lambda dtype=_dtype: {"data": _data((2, 2, 13, 9, 20), dtype, 91)}, arguments=lambda t, out=_out, mode=_mode: ((t["data"], out, mode), {}))


def _gather_inputs(dtype, axis, blend):
    def build():
        data = _data((3, 2, 10, 12, 14), dtype, 92)
        length = data.shape[2 + axis]
        g = torch.Generator().manual_seed(93)
        t = {"data": data, "lower": torch.randint(0, length, (3, length), generator=g, dtype=I32), "active": torch.tensor([1, 0, 1], dtype=U8)}
        if blend:
            t["upper"] = torch.randint(0, length, (3, length), generator=g, dtype=I32)
            t["weight"] = torch.rand(3, length, generator=g)
        return t

    return build


for _dtype, _axis, _blend in ((F32, 0, True), (F32, 1, True), (F32, 2, True), (F16, 2, True), (I16, 2, False), (I16, 0, False)):
    _add(id=f"axis_gather_lerp-{str(_dtype).split('.')[-1]}-axis{_axis}-{'blend' if _blend else 'gather'}", method="axis_gather_lerp",
         inputs=_gather_inputs(_dtype, _axis, _blend), also=_kept_row_is_the_input,
         arguments=lambda t, axis=_axis: ((t["data"], axis, t["lower"], t.get("upper"), t.get("weight"), t["active"]), {}))

for _dtype in (F32, F64, BF16, U8, I16, I64):
    for _axes in ([0, 2], [0, 1, 2]):
        _add(id=f"flip3d-{str(_dtype).split('.')[-1]}-{''.join(str(a) for a in _axes)}", method="flip3d",
             inputs=lambda dtype=_dtype: {"data": _data((3, 2, 7, 9, 11), dtype, 101)}, arguments=lambda t, axes=_axes: ((t["data"], axes), {}),
             also=lambda got, cpu, axes=_axes: exact(torch.flip(cpu["data"], [2 + a for a in axes]), got[0], "torch.flip"))
_add(id="flip3d-per_element", method="flip3d",
     inputs=lambda: {"data": _data((3, 2, 7, 9, 11), F32, 101), "flags": torch.tensor([[1, 0, 1], [0, 0, 0], [0, 1, 0]], dtype=U8)},
     arguments=lambda t: ((t["data"],), {"per_element": t["flags"]}))

for _mode in ("constant", "reflect", "replicate", "circular"):
    for _dtype in (F32, I16, U8, F64):
        _fill = (3.0 if _dtype == U8 else -3.0) if _mode == "constant" else 0.0
        _add(id=f"pad3d-{_mode}-{str(_dtype).split('.')[-1]}", method="pad3d", inputs=lambda dtype=_dtype: {"data": _data((2, 3, 6, 9, 11), dtype, 103)},
             arguments=lambda t, mode=_mode, fill=_fill: ((t["data"], (2, 5, 0, 3, 4, 1), mode), {"fill": fill}))
_add(id="pad3d-per_element_constants", method="pad3d",
     inputs=lambda: {"data": _data((3, 2, 5, 6, 7), F32, 105), "fills": torch.tensor([0.25, -7.0, 1e9])},
     arguments=lambda t: ((t["data"], (1, 2, 3, 0, 0, 4)), {"fill_per_element": t["fills"]}))
_add(id="pad3d-reflect-more_than_one_block_per_row", method="pad3d", inputs=lambda: {"data": _data((1, 1, 40, 50, 300), I16, 107)},
     arguments=lambda t: ((t["data"], (3, 3, 7, 7, 33, 31), "reflect"), {}))

# unique_labels demands 16 bytes of its data: the engine re-aligns a shifted view (a copy), same table
for _dtype in (U8, I8, I16):
    _add(id=f"unique_labels-{str(_dtype).split('.')[-1]}", method="unique_labels",
         inputs=lambda dtype=_dtype: {"data": torch.randint(0, 5, (2, 1, 17, 19, 23), generator=torch.Generator().manual_seed(301)).to(dtype)},
         arguments=lambda t: ((t["data"],), {}), also=lambda got, cpu: exact(torch.unique(cpu["data"]).double(), got[0], "torch.unique"))


# ---------------------------------------------------------------------------------------------------------------------
# Motion's k-space composite, against the float64 FFT route (test_kspace_segment_mix_matches_the_fft_route)
# ---------------------------------------------------------------------------------------------------------------------
def _fft_route(segments, bounds):
    spectrum = torch.fft.fftn(segments[0].double(), dim=(-3, -2, -1))
    for s in range(1, len(segments)):
        spectrum[:, :, bounds[s] : bounds[s + 1]] = torch.fft.fftn(segments[s].double(), dim=(-3, -2, -1))[:, :, bounds[s] : bounds[s + 1]]
    return torch.fft.ifftn(spectrum, dim=(-3, -2, -1)).real


def _kspace_bar(want, got, what):  # two float32 evaluations of the same sums against the float64 DFT: <= 1e-5 of the magnitude (4)
    absmax(1e-5 * 4)(want, got.double(), what)


for _shape, _bounds in (((2, 1, 12, 6, 5), [0, 4, 8, 12]), ((1, 2, 16, 8, 8), [0, 8, 16]), ((1, 1, 150, 7, 9), [0, 37, 74, 111, 150]),
                        ((1, 1, 260, 4, 36), [0, 130, 260]), ((3, 1, 9, 12, 1), [0, 9]), ((1, 1, 33, 20, 20), [0, 0, 11, 33])):
    _add(id=f"kspace_segment_mix-{'x'.join(str(s) for s in _shape)}", method="kspace_segment_mix", skewed=("segments",), bar=_kspace_bar,
         inputs=lambda shape=_shape, bounds=_bounds: {"segments": _segments(shape, len(bounds) - 1, 201)},
         arguments=lambda t, bounds=_bounds: ((t["segments"], bounds, F32), {}),
         reference=lambda oracle, cpu, hip, bounds=_bounds: [_fft_route(cpu["segments"], bounds)], skew_bits=False)
_add(id="kspace_segment_mix-inactive_element", method="kspace_segment_mix", skewed=("segments",), bar=_kspace_bar, skew_bits=False,
     inputs=lambda: {"segments": _segments((3, 2, 12, 6, 8), 2, 203), "active": torch.tensor([1, 0, 1], dtype=U8)},
     arguments=lambda t: ((t["segments"], [0, 5, 12], F32), {"active": t["active"]}),
     compared=lambda outs: [outs[0][[0, 2]]], untouched=lambda outs: [outs[0][1]],  # the kernel promises not to touch an inactive element's rows
     reference=lambda oracle, cpu, hip: [_fft_route(cpu["segments"], [0, 5, 12])])


# ---------------------------------------------------------------------------------------------------------------------
# the patch aggregator: caller-owned accumulators, written in place
# ---------------------------------------------------------------------------------------------------------------------
def _patch_inputs(dtype, mode, volume=(20, 18, 22), patch=(8, 8, 8), count=6, channels=2, start=(3, 2, 5)):
    def build():
        g = torch.Generator().manual_seed(6)
        values = torch.randn(count, channels, *patch, generator=g) if dtype.is_floating_point else torch.randint(0, 7, (count, channels, *patch), generator=g)
        t = {"out": torch.zeros(channels, *volume, dtype=dtype), "patches": values.to(dtype)}
        if mode != "crop":
            t["weight_sum"] = torch.zeros(channels, *volume, dtype=dtype)
        if mode == "hann":
            t["windows"] = [torch.hann_window(extent + 2, periodic=False)[1:-1].float() for extent in patch]
        return t

    # the bounding box of the placements starts inside the volume; patches overlap, the last one is clipped to a part of itself
    placements = [((start[0] + (3 * n) % 9, start[1] + (5 * n) % 7, start[2] + (2 * n) % 8), (0, 0, 0), patch) for n in range(count - 1)]
    placements.append(((start[0] + 1, start[1] + 1, start[2] + 1), (2, 1, 3), tuple(extent - 3 for extent in patch)))
    if count == 1:
        placements = [((0, 0, 0), (0, 0, 0), patch)]
    return build, placements


def _add_patches(name, dtype, mode, **sizes):
    build, placements = _patch_inputs(dtype, mode, **sizes)
    _add(id=f"patch_accumulate-{mode}-{name}", method="patch_accumulate", inputs=build, skewed=("out", "weight_sum", "patches"), owned=False,
         arguments=lambda t: ((t["out"], t.get("weight_sum"), t["patches"], placements, mode), {"windows": t.get("windows")}),
         outputs=lambda result, t: [t["out"]] + ([t["weight_sum"]] if "weight_sum" in t else []))


for _mode in ("crop", "average", "hann"):
    for _dtype, _name in ((F32, "f32"), (F16, "f16"), (BF16, "bf16"), (F64, "f64")):
        _add_patches(_name, _dtype, _mode)
_add_patches("i16", I16, "crop")
# more than 256 x 64 blocks of 256 box voxels (4 194 304): the grid-stride loop runs
_add_patches("grid_stride", F32, "average", volume=(162, 162, 162), patch=(162, 162, 162), count=1, channels=1)

assert len({case.id for case in CASES}) == len(CASES), "case ids must be unique"
