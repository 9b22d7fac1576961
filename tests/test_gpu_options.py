"""kanode_set_option / kanode_get_option through a real handle (csrc/kanode_options.hpp's table behind the C-ABI):
every name of kanode._lib.OPTIONS reads the default include/kanode.h documents, a legal value round-trips, an illegal
one raises and leaves the old value, kanode_last_error carries the exact refusal text, and POINTWISE_TABLE = 1 is
refused where the handle has no table (fp32) and accepted where it has one (fp64 Fisher-KPP).  Three handles of the
smallest shapes the constructor accepts; no kernel is launched beyond what kanode_create does.  The table itself, row
by row, is tests/host/options_test.cpp."""
import pytest
import torch

from gpu_util import device

import kanode
from kanode import _lib as L

pytestmark = pytest.mark.gpu

# include/kanode.h: (default, a legal value that is not the default, an illegal value); pointwise_table's default
# depends on the handle (1 where admissible) and is stated per handle below; last_adjoint and last_eval are read-only
DOC = {
    "fused_step": (1, 0, 2), "fused_solve": (1, 0, -1), "fused_solve_cap": (0, 1 << 20, (1 << 20) + 1),
    "grid_rhs": (0, 1 << 24, (1 << 24) + 1), "grid_vjp": (0, 2048, 2049), "grid_adj_step": (0, 2048, 2049),
    "adj_step_rows": (1, 0, 2), "pair_vjp": (1, 0, 2), "pair_fuse": (1, 0, 2), "pair_persist": (1, 0, 2),
    "pair_persist_s": (0, 16, 5), "adj_fused_finish": (0, 1, 2), "pair_persist_max_wg": (0, 7, -1),
    "pair_persist_abort": (0, 1, 2), "chain_wide": (1, 0, 2), "record_adjoint_steps": (0, 1, 2),
    "fk_device_loop": (1, 0, 2), "fsens_wide": (0, 2, 3), "train_any_chain": (0, 1, 2),
}
TABLE_DEFAULT = {"chain64": 0, "fk64": 1, "fk32": 0}


@pytest.fixture(scope="module")
def handles():
    dev = device()
    chain = [kanode.LayerCfg(2, 3, 3), kanode.LayerCfg(3, 2, 3)]
    fk = dict(rhs_kind="pointwise_periodic_laplacian", nx=8, diffusion=0.01, dx=1.0 / 7, device=dev)
    return {"chain64": kanode.KanodeHandle(chain, dtype=torch.float64, device=dev),
            "fk64": kanode.KanodeHandle([kanode.LayerCfg(1, 1, 3)], dtype=torch.float64, **fk),
            "fk32": kanode.KanodeHandle([kanode.LayerCfg(1, 1, 3)], dtype=torch.float32, **fk)}


def _last_error(hd):
    return L.lib().kanode_last_error(hd._h).decode()


@pytest.mark.parametrize("which", ["chain64", "fk64", "fk32"])
def test_defaults_round_trip_and_refusal(handles, which):
    hd = handles[which]
    assert set(L.OPTIONS) == set(DOC) | {"pointwise_table", "last_adjoint", "last_eval"}
    assert hd.get_option("pointwise_table") == TABLE_DEFAULT[which]
    assert hd.get_option("last_adjoint") == 0   # KANODE_ADJ_NONE: no adjoint on this handle yet
    assert hd.get_option("last_eval") == L.EVAL_NONE == 0   # no evaluation on this handle yet
    for name, (dflt, legal, illegal) in DOC.items():
        assert hd.get_option(name) == dflt, name
        hd.set_option(name, legal)
        assert hd.get_option(name) == legal, name
        with pytest.raises(kanode.KanodeError, match="invalid argument"):
            hd.set_option(name, illegal)
        assert hd.get_option(name) == legal, name   # a refused set leaves the old value
        hd.set_option(name, dflt)
        assert hd.get_option(name) == dflt, name
    with pytest.raises(kanode.KanodeError, match="LAST_ADJOINT is read-only"):
        hd.set_option("last_adjoint", 1)
    assert hd.get_option("last_adjoint") == 0
    with pytest.raises(kanode.KanodeError, match="LAST_EVAL is read-only"):
        hd.set_option("last_eval", 1)
    assert hd.get_option("last_eval") == 0
    # ids on either side of the enum
    for bad in (0, 23):
        assert L.lib().kanode_get_option(hd._h, bad) == -1
        assert L.lib().kanode_set_option(hd._h, bad, 0) == L.ERR_INVALID_ARG
        assert _last_error(hd) == f"unknown option {bad}"


def test_refusal_messages(handles):
    hd = handles["chain64"]
    for name, value, text in [("fused_step", 2, "FUSED_STEP takes 0 or 1"),
                              ("grid_vjp", 2049, "GRID_VJP takes 0..2048"),
                              ("pair_persist_s", 2, "PAIR_PERSIST_S takes 0 (default), 4, 8 or 16")]:
        assert L.lib().kanode_set_option(hd._h, L.OPTIONS[name], value) == L.ERR_INVALID_ARG
        assert _last_error(hd) == text


def test_pointwise_table_needs_the_table(handles):
    f32, f64 = handles["fk32"], handles["fk64"]
    with pytest.raises(kanode.KanodeError, match="unsupported configuration"):
        f32.set_option("pointwise_table", 1)
    assert _last_error(f32) == "POINTWISE_TABLE needs a pointwise f64 RHS with rbf/rswaf basis and even nx"
    assert f32.get_option("pointwise_table") == 0
    f32.set_option("pointwise_table", 0)   # 0 is always accepted
    f64.set_option("pointwise_table", 0)
    assert f64.get_option("pointwise_table") == 0
    f64.set_option("pointwise_table", 1)
    assert f64.get_option("pointwise_table") == 1
    with pytest.raises(kanode.KanodeError, match="POINTWISE_TABLE takes 0 or 1"):
        f64.set_option("pointwise_table", 2)
    assert f64.get_option("pointwise_table") == 1
