"""hip.py's one allocator and its one rule for recorded steps, on the host: every device tensor of the module comes from
hip._new, which keeps it referenced while a hip.holding() block is open; a launch deferred to a plan's inline section
(LaunchPlan.defer_side) is kept, with everything its closure references, until the section is joined or the recording ends.
CPU tensors; the library's calls are stand-ins that return 0."""
import ast
import gc
import os
import weakref

import pytest
import torch

from rec_pangu_amd import hip

CPU = torch.device("cpu")


def _dropped():
    """a tensor from hip._new that its caller drops at once -> a weak reference to it"""
    return weakref.ref(hip._new((16,), torch.float32, CPU))


def test_a_dropped_tensor_lives_until_its_holding_block_ends():
    assert not hip.holding.active()
    with hip.holding() as items:
        assert hip.holding.active()
        ref = _dropped()
        gc.collect()
        assert ref() is not None and any(t is ref() for t in items)
    assert not hip.holding.active()
    del items
    gc.collect()
    assert ref() is None


def test_outside_a_holding_block_a_dropped_tensor_dies_at_once():
    ref = _dropped()
    assert ref() is None
    like = weakref.ref(hip._new_like(torch.zeros(3, 5)))
    assert like() is None


def test_nested_holding_blocks_keep_their_own_tensors():
    with hip.holding() as outer:
        a = _dropped()
        with hip.holding() as inner:
            b = _dropped()
            assert [t is b() for t in inner] == [True] and [t is a() for t in outer] == [True]
        del inner
        gc.collect()
        assert b() is None and a() is not None and hip.holding.active()
        c = _dropped()
        assert [t is x() for t, x in zip(outer, (a, c))] == [True, True]
    assert not hip.holding.active()


def test_a_holding_block_is_closed_behind_an_exception():
    try:
        with hip.holding():
            with hip.holding():
                raise KeyError("inside")
    except KeyError:
        pass
    assert not hip.holding.active()


def test_a_workspace_is_held_like_any_other_tensor(monkeypatch):
    class Lib:
        @staticmethod
        def rp_linear_wgrad_workspace_bytes(m, n, k, out):
            out._obj.value = m * n * k
            return 0

    monkeypatch.setattr(hip, "lib", lambda: Lib)
    with hip.holding() as items:
        ws, nbytes = hip._workspace("linear_wgrad", 2, 3, 4, device=CPU)
        assert nbytes == 24 and ws.dtype == torch.uint8 and ws.numel() == 24 and items[-1] is ws
        given, nbytes = hip._workspace("linear_wgrad", 2, 3, 4, device=CPU, given=ws)
        assert given is ws and nbytes == 24 and len(items) == 1
        small = torch.empty(8, dtype=torch.uint8)
        fresh, _ = hip._workspace("linear_wgrad", 2, 3, 4, device=CPU, given=small)
        assert fresh is not small and fresh.numel() == 24 and len(items) == 2


class _Target:
    pass


def _plan_stubs(monkeypatch, recording=True):
    class Lib:
        def __getattr__(self, name):  # rp_plan_join, rp_plan_end, rp_plan_info, rp_plan_section ...: all succeed
            return lambda *args: 0

    monkeypatch.setattr(hip, "lib", lambda: Lib())
    monkeypatch.setattr(hip.LaunchPlan, "is_recording", staticmethod(lambda: recording))
    monkeypatch.setattr(hip.LaunchPlan, "_deferred", [])
    monkeypatch.setattr(hip.LaunchPlan, "_kept", [])


def _defer(calls):
    """defer a closure over a fresh object, drop both -> weak references to (the closure, the object)"""
    target = _Target()

    def fn():
        calls.append(target)

    hip.LaunchPlan.defer_side(fn)
    return weakref.ref(fn), weakref.ref(target)


def test_a_deferred_launch_is_kept_until_the_join(monkeypatch):
    _plan_stubs(monkeypatch)
    calls = []
    fn, target = _defer(calls)
    gc.collect()
    assert fn() is not None and target() is not None
    hip.LaunchPlan.run_deferred()  # issued: still kept (it runs beside what is recorded until the join)
    assert len(calls) == 1 and calls.pop() is target()
    gc.collect()
    assert fn() is not None and target() is not None
    hip.LaunchPlan.join()
    gc.collect()
    assert fn() is None and target() is None and not calls


def test_the_join_issues_a_deferred_launch_and_lets_it_go(monkeypatch):
    _plan_stubs(monkeypatch)
    calls = []
    fn, target = _defer(calls)
    hip.LaunchPlan.join()
    assert len(calls) == 1
    del calls[:]
    gc.collect()
    assert fn() is None and target() is None


@pytest.mark.parametrize("recording", [True, False])
def test_the_end_of_a_recording_lets_a_deferred_launch_go_without_a_join(monkeypatch, recording):
    """nobody joined the inline section: end() does it while the library still records (the launch is issued), and drops the
    launch unissued when the recording is already over (a capture that failed)"""
    _plan_stubs(monkeypatch, recording)
    calls = []
    fn, target = _defer(calls)
    hip.LaunchPlan().end()
    assert len(calls) == int(recording)
    del calls[:]
    gc.collect()
    assert fn() is None and target() is None


# ---- the invariant itself: nobody in hip.py allocates beside _new ------------------------------------------------------
ALLOCATORS = {"empty", "zeros", "empty_like", "zeros_like", "full"}
# functions whose tensor lives on the HOST (no stream runs beside it, no capture pool holds it)
HOST_ONLY = {
    "adam_step_scalars_range",  # the [n, 2] float32 table of per-step scalars, filled by a C call on the host
}


def test_every_device_tensor_of_hip_py_comes_from_new():
    path = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "hip.py")
    with open(path) as fh:
        tree = ast.parse(fh.read())
    found = []

    def walk(node, owner):
        for child in ast.iter_child_nodes(node):
            inside = child.name if isinstance(child, (ast.FunctionDef, ast.ClassDef)) and owner is None else owner
            if isinstance(child, ast.Call) and isinstance(child.func, ast.Attribute) and child.func.attr in ALLOCATORS \
                    and isinstance(child.func.value, ast.Name) and child.func.value.id == "torch":
                found.append((owner, child.func.attr, child.lineno))
            walk(child, inside)

    walk(tree, None)
    assert ("_new", "empty") in {(o, a) for o, a, _ in found}  # (the walk sees what it is looking for)
    stray = [f for f in found if f[0] != "_new" and f[0] not in HOST_ONLY]
    assert not stray, f"hip.py allocates beside _new (module-level function, torch call, line): {stray}"
    assert {o for o, _, _ in found} == {"_new"} | HOST_ONLY  # (no stale entry in the allow-list)
