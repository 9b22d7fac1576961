"""CPU-side checks of the ensemble entry for every small chain (kanode_fit_ensemble_tsit5) and of
EnsembleTrainer(device_loop=...): the header's declarations, the bindings, the exported symbols and their names, the
null handle, the keyword's values and the host path without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

import kanode
from kanode import _lib as L
from oracle import oracle as O
from oracle.oracle_rhs import OracleChainRHS

HEADER = os.path.join(ROOT, "include", "kanode.h")
ENTRIES = ["kanode_fit_ensemble_group", "kanode_fit_ensemble_supported", "kanode_fit_ensemble_tsit5"]
TS = [0.1 * i for i in range(35)]


def test_header_bindings_and_exports():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"int32_t\s+kanode_fit_ensemble_supported\(const kanode_handle\* h, int64_t batch\);", src)
    assert re.search(r"int64_t\s+kanode_fit_ensemble_group\(const kanode_handle\* h, int64_t batch, double t0, double tf,"
                     r"\s*int64_t n_save,\s*int64_t n_save_test, const kanode_solver_options\* opt\);", src)

    def args(name):
        decl = re.search(r"kanode_status\s+" + name + r"\s*\((.*?)\)\s*;", src, flags=re.S).group(1)
        return [re.sub(r"\s+", " ", a.strip()) for a in decl.split(",")]
    assert args("kanode_fit_ensemble_tsit5") == args("kanode_train_ensemble_tsit5")
    sig = {n: (r, a) for n, r, a in L.SIGNATURES}
    assert sorted(n for n in sig if "fit_ensemble" in n) == ENTRIES
    assert sig["kanode_fit_ensemble_tsit5"] == sig["kanode_train_ensemble_tsit5"]
    assert sig["kanode_fit_ensemble_tsit5"][1] is L._ENSEMBLE_ARGS
    assert sig["kanode_fit_ensemble_supported"] == sig["kanode_train_supported"]
    assert len(sig["kanode_fit_ensemble_group"][1]) == 7
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert sorted(n for n in exported if "fit_ensemble" in n) == ENTRIES
    assert not [n for n in ENTRIES if "train" in n or "_wg" in n or "any_chain" in n]
    # the header no longer calls these ensembles out of scope, and points to the new entry from the old one
    whole = open(HEADER).read()
    assert "replicas of a general chain are out of scope" not in whole
    old = whole[whole.index("--- ensemble training: n_replicas"):whole.index("kanode_status kanode_train_ensemble_tsit5(")]
    assert "kanode_fit_ensemble_tsit5" in old
    assert max(L.OPTIONS.values()) == 22                          # (no new handle option)


def test_null_handle():
    lib = L.lib()
    assert lib.kanode_fit_ensemble_supported(None, 1) == 0
    opts = kanode.Tsit5Options().to_c()
    assert lib.kanode_fit_ensemble_group(None, 1, 0.0, 3.5, 35, 0, opts) == 0
    assert lib.kanode_fit_ensemble_group(None, 1, 0.0, 3.5, 35, 0, None) == 0
    done, stop = (L.C.c_int64 * 1)(), (L.C.c_int32 * 1)()
    eta, bt = (L.C.c_double * 1)(1e-3), (L.C.c_double * 2)(0.9, 0.999)
    st = lib.kanode_fit_ensemble_tsit5(None, 1, None, None, None, None, 1, 0.0, 3.5, None, 0, None, 0.0, None, 0, None,
                                       None, eta, None, 0.9, 0.999, 1e-8, bt, 1, None, None, None, None, None, done,
                                       stop, None)
    assert st == L.ERR_INVALID_ARG != L.OK


def problem(R=3):
    rng = np.random.default_rng(11)
    specs = [O.LayerSpec(2, 4, 5, "tanh_fast"), O.LayerSpec(4, 2, 5, "tanh_fast")]   # a pruned LV net
    p = rng.uniform(-0.3, 0.3, 96)
    u0 = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 2)))
    X = torch.as_tensor(rng.uniform(0.5, 2.0, (35, 1, 2)))
    p0 = torch.as_tensor(np.stack([p * s for s in (1.0, 0.9, 1.1)][:R]))
    return OracleChainRHS(specs), u0, X, p0


def test_bad_device_loop_raises():
    rhs, u0, X, p0 = problem()
    for bad in ("all", "", None, 1):
        with pytest.raises(ValueError, match="device_loop"):
            kanode.EnsembleTrainer(rhs, u0, (0.0, 3.5), TS, X, p0, device_loop=bad)
    assert kanode.EnsembleTrainer(rhs, u0, (0.0, 3.5), TS, X, p0).device_loop == "default"


def test_device_loop_any_without_a_gpu_is_the_host_path():
    """On the oracle RHS "any" changes nothing: run() is the host path and equals the default bit for bit; the
    members and member(r) carry the keyword."""
    rhs, u0, X, p0 = problem()
    etas, lams = [1e-3, 5e-4, 2e-3], [0.0, 5e-4, 1e-3]
    a = kanode.EnsembleTrainer(rhs, u0, (0.0, 3.5), TS, X, p0, eta=etas, sparse_reg=lams, device_loop="any")
    b = kanode.EnsembleTrainer(rhs, u0, (0.0, 3.5), TS, X, p0, eta=etas, sparse_reg=lams)
    oa, ob = a.run(2, record=True), b.run(2, record=True)
    assert a.last_run == "host" == b.last_run
    for key in ("loss", "grad", "p_before", "counts"):
        assert torch.equal(oa[key], ob[key]), key
    assert torch.equal(a.p, b.p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    assert a.bp == b.bp and a.history == b.history and oa["iters_done"] == ob["iters_done"] == [2, 2, 2]
    assert not torch.equal(a.p[0], a.p[1])
    for r in range(3):
        assert a._members[r].device_loop == "any" and b._members[r].device_loop == "default"
        assert a.member(r).device_loop == "any" and b.member(r).device_loop == "default"
