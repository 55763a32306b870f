"""The one interface of the four precisions (engine.get_engine / engine.EngineWorkspace), checked on the host: it is
complete for every registered name, the three kernel sequences take the same arguments whatever the engine, and the fp32
engine's answers are the documented no-ops."""
import inspect

import pytest
import torch

from cdml_amd import engine, engine_bf16, engine_f16x2, engine_x3

NAMES = ("f32", "bf16", "f32x3", "f32x3-3", "f16x2")
HOOKS = ("tail_operands", "miner_operands", "optimizer_operands", "enable_row_gradient", "row_gradient", "scales_due",
         "observe_weights", "observe_gradients", "scales_state", "load_scales")


def params(fn, drop=()):
    return [(p.name, p.kind, p.default) for p in inspect.signature(fn).parameters.values() if p.name not in drop]


@pytest.mark.parametrize("name", NAMES)
def test_interface_is_complete(name):
    E = engine.get_engine(name)
    assert E.name == name and issubclass(E.Workspace, engine.EngineWorkspace)
    for f in (E.layout, E.workspace, E.refresh_weights, E.tower_forward, E.tower_backward):
        assert callable(f)
    L = E.layout(300, 300, 64)
    w = E.Workspace.WIDTHS
    assert (L.F, L.H, L.D) == (300, 300, 64) and not (L.Fp % w or L.Hp % w or L.Dp % w)
    for hook in HOOKS:          # an override keeps the base class's arguments
        assert params(getattr(E.Workspace, hook)) == params(getattr(engine.EngineWorkspace, hook)), hook
    kinds = [p.kind for p in inspect.signature(E.Workspace.__init__).parameters.values()]
    assert (inspect.Parameter.VAR_KEYWORD in kinds) == (name not in ("f32x3", "f32x3-3"))      # x3 has every option
    assert [n for n, _, _ in params(E.Workspace.__init__)][:4] == ["self", "layout", "n_rows", "device"]
    assert inspect.signature(E.Workspace.__init__).parameters["backward"].default is True


def test_the_registry_maps_the_names_to_the_existing_modules():
    got = {n: (engine.get_engine(n).layout, engine.get_engine(n).Workspace, engine.get_engine(n).rows,
               engine.get_engine(n).table_dtype, engine.get_engine(n).ws_args) for n in NAMES}
    assert got == {
        "f32": (engine.TowerLayout, engine.TowerWorkspace, 1, torch.float32, {}),
        "bf16": (engine_bf16.layout_bf16, engine_bf16.TowerWorkspaceBF16, 64, torch.float16, {}),
        "f32x3": (engine_x3.layout_x3, engine_x3.TowerWorkspaceX3, 128, torch.float32, {"products": 6}),
        "f32x3-3": (engine_x3.layout_x3, engine_x3.TowerWorkspaceX3, 128, torch.float32, {"products": 3}),
        "f16x2": (engine_x3.layout_x3, engine_f16x2.TowerWorkspaceH2, 128, torch.float32, {})}
    assert [engine.get_engine(n).Workspace.INFERENCE for n in NAMES] == ["f32", "bf16", "f32x3", "f32x3", "f32"]


@pytest.mark.parametrize("name", ["auto", None, "fp8", "F32"])
def test_an_unknown_name_is_refused_with_the_constructors_words(name):
    with pytest.raises(ValueError, match="^precision must be 'auto', 'f32', 'f32x3', 'f16x2' or 'bf16'$"):
        engine.get_engine(name)


def test_the_kernel_sequences_take_the_same_arguments():
    ref = engine.get_engine("f32x3")
    assert [n for n, _, _ in params(ref.tower_forward)] == ["p", "ws", "normalize"]
    assert [(n, d) for n, _, d in params(ref.tower_backward)[2:]] == [("after_w1", None), ("w1_chunks", 1),
                                                                      ("after_w1_chunk", None)]
    for name in NAMES:
        E = engine.get_engine(name)
        # (the fp32 MFMA alone runs on part of a workspace: its extra ``n_rows``, a keyword)
        drop = ("n_rows",) if name == "f32" else ()
        assert params(E.refresh_weights) == params(ref.refresh_weights), name
        assert params(E.tower_forward, drop) == params(ref.tower_forward), name
        assert params(E.tower_backward, drop) == params(ref.tower_backward), name
    for fn in (engine.tower_forward, engine.tower_backward):
        assert inspect.signature(fn).parameters["n_rows"].default is None


def test_fp32_defaults_are_no_ops():
    ws = engine.EngineWorkspace()
    assert ws.tail_operands() == ({}, False) and ws.tail_operands(indexed=True) == ({}, False)
    assert ws.miner_operands() is None and ws.optimizer_operands() is None
    assert ws.enable_row_gradient(None) is None and ws.W1n is None
    assert ws.scales_due() is False and ws.scales_due(0) is False and ws.scales_due(64) is False
    assert ws.observe_weights(None) is False and ws.observe_gradients(None) is None      # (False: the caller refreshes)
    assert ws.scales_state() is None
    assert ws.load_scales(None, {"w1": 2.0}) is False and ws.load_scales(None, None) is False
    assert (ws.h1_bits, ws.xk, ws.scales, ws.kint, ws.tail_done, ws.dz2_planes_done) == (None, None, None, False, False, False)
    assert engine.refresh_weights(None, None) is None                  # no operand copies on the fp32 MFMA
    for hook in HOOKS:                                                 # fp32 overrides none of them
        assert getattr(engine.TowerWorkspace, hook) is getattr(engine.EngineWorkspace, hook)


def test_auto_precision():
    assert engine.auto_precision(torch.float16, 100) == "bf16"
    assert [engine.auto_precision(torch.float32, r) for r in (128, 384, 192, 100)] == ["f32x3", "f32x3", "f32", "f32"]
    assert [engine.auto_precision(torch.float32, b, 256) for b in (256, 128, 512)] == ["f32x3", "f32", "f32x3"]


def test_workspace_options_reach_only_the_engines_that_have_them(monkeypatch):
    """Engine.workspace hands every option to the constructor; the ones an engine does not have end in its **keywords."""
    for name, kept in (("f32", ()), ("bf16", ()), ("f16x2", ("planes_in",)), ("f32x3", ("planes_in", "kint", "fc2_single_pass"))):
        named = inspect.signature(engine.get_engine(name).Workspace.__init__).parameters
        assert [k for k in ("planes_in", "kint", "fc2_single_pass") if k in named] == list(kept), name
    seen = {}
    for name in NAMES:
        E = engine.get_engine(name)
        monkeypatch.setattr(E.Workspace, "__init__", lambda self, *a, _n=name, **kw: seen.__setitem__(_n, kw))
        E.workspace(None, 128, "cpu", backward=False, planes_in=False)
    assert seen["f32x3-3"] == {"backward": False, "products": 3, "planes_in": False}
    assert seen["f32x3"]["products"] == 6 and seen["f32"] == seen["f16x2"] == {"backward": False, "planes_in": False}
