"""The table of tests/workspace_cases.py against the code, without a GPU: a new entry with a workspace, or a new
module with a `_lib.Workspace`, cannot stay out of tests/test_gpu_workspace_state.py."""
import ctypes as C
import os

import pytest
import torch

from tests import workspace_cases as W


def test_every_ws_bytes_query_of_the_header_is_covered():
    declared = W.declared_ws_queries()
    assert len(declared) >= 12 and "l2hmc_gauge_mcmc_step_ws_bytes" in declared
    covered = {q for op in W.OPS.values() for q in op.covers}
    assert covered <= set(declared), sorted(covered - set(declared))
    assert not set(declared) - covered, f"no operation of the table fills the workspace of {sorted(set(declared) - covered)}"


def test_every_module_with_a_workspace_is_covered():
    modules = W.modules_with_a_workspace()
    assert {"gauge_dynamics", "network"} <= set(modules)
    covered = {m for op in W.OPS.values() for m in op.modules}
    assert not set(modules) - covered, f"no operation of the table goes through {sorted(set(modules) - covered)}"
    pkg = os.path.join(W.ROOT, "l2hmc_amd")
    for module, name in W.BARE_EMPTY_SITES.items():     # the bare torch.empty sites: reached through their C entries
        assert os.path.exists(os.path.join(pkg, module + ".py")) and name in W.OPS and not W.OPS[name].modules


def test_the_table_is_well_formed():
    assert len(W.OPS) == len({op.build for op in W.OPS.values()})
    for op in W.OPS.values():
        assert op.covers and callable(op.build), op.name
        assert op.stale_from in W.OPS and op.stale_from != op.name, op.name
    for kind, ladder in W.CAPTURED:
        assert f"step_{kind}" + ("_ladder" if ladder else "") in W.OPS
    assert ("cut_batch", False) in W.CAPTURED and any(lad for _, lad in W.CAPTURED)


@pytest.mark.parametrize("pattern", W.PATTERNS)
def test_the_poisoning_helper_fills_the_whole_buffer(pattern, monkeypatch):
    from l2hmc_amd import _lib
    cpu = torch.device("cpu")
    plain = _lib.Workspace.get
    with W.poisoned(monkeypatch, pattern) as shared:
        a, b = _lib.Workspace(), _lib.Workspace()
        ptr, n = a.get(1000, cpu)
        assert n == 1000 and shared.buf.data_ptr() == ptr and shared.gets == 1
        assert bool((shared.buf == pattern).all())
        words = shared.buf[:1000 - 1000 % 4].view(torch.int32)
        assert bool((words == {0x00: 0, 0xFF: -1, 0x7F: 0x7F7F7F7F}[pattern]).all())
        if pattern == 0xFF:
            assert bool(shared.buf[:1000].view(torch.float32).isnan().all())
        if pattern == 0x7F:
            assert float(shared.buf[:4].view(torch.float32)) == pytest.approx(3.39e38, rel=1e-2)
        shared.buf.fill_(0x11)                           # what a call leaves behind ...
        ptr2, n2 = b.get(300, cpu)                       # ... is gone when the next one (of ANY Workspace) starts
        assert (ptr2, n2) == (ptr, n) and bool((shared.buf == pattern).all())
        ptr3, n3 = a.get(5000, cpu)                      # grown: filled to its new end
        assert n3 == 5000 and shared.buf.numel() == 5000 and bool((shared.buf == pattern).all())
        shared.pattern = None                            # left alone
        shared.buf.fill_(0x22)
        a.get(100, cpu)
        assert bool((shared.buf == 0x22).all())
    assert _lib.Workspace.get is plain


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_the_cut_batch_chooser_returns_a_three_part_plan(cus):
    B = W.cut_batch_chains(cus)
    parts = W.step_plan(2 * B, cus)
    assert W.is_cut_in_three(parts), parts
    assert sum(r for r, _ in parts) == 2 * B and all(r % 2 == 0 and r > 0 for r, _ in parts)
    assert B > 16 * cus // 2                             # more than one round of 16-row workgroups
    assert not any(W.is_cut_in_three(W.step_plan(2 * b, cus)) for b in range(max(1, B - 64), B))
    if cus == 256:
        assert B <= 6199                                 # DESIGN.md section 7 names 6199 chains on 256 CUs
    # host logic only: the query takes no device pointer
    from l2hmc_amd import _lib
    rows, rpw = (C.c_int64 * 3)(), (C.c_int32 * 3)()
    assert _lib.lib().l2hmc_gauge_step_plan(2 * B, cus, rows, rpw) == 3
