"""CPU-side checks of KANODE_OPT_TRAIN_ANY_CHAIN and Trainer(device_loop=...): the option's id and documented
default, the keyword's values, the host loop without a GPU, and the unchanged set of exported entry points."""
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
TRAIN_ENTRIES = ["kanode_train_ensemble_tsit5", "kanode_train_forward_ensemble_tsit5", "kanode_train_forward_supported",
                 "kanode_train_forward_tsit5", "kanode_train_supported", "kanode_train_tsit5"]


def test_option_id_and_documented_default():
    src = open(HEADER).read()
    body = re.search(r"typedef enum \{([^}]*)\} kanode_option;", src, flags=re.S).group(1)
    assert re.search(r"KANODE_OPT_TRAIN_ANY_CHAIN\s*=\s*21\b", body)
    assert L.OPTIONS["train_any_chain"] == 21 == L.OPT_TRAIN_ANY_CHAIN
    # (one option follows it: the read-only LAST_EVAL = 22)
    assert max(L.OPTIONS.values()) == 22 == L.OPT_LAST_EVAL and len(set(L.OPTIONS.values())) == len(L.OPTIONS)
    assert re.search(r"KANODE_OPT_TRAIN_ANY_CHAIN \(default 0\)", src)


def test_exports_are_unchanged_in_name():
    """The feature is an option and a keyword: no entry point was added or renamed."""
    out = subprocess.run(["nm", "-D", "--defined-only", kanode.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = set(re.findall(r"\sT\s+(kanode_\w+)", out))
    assert sorted(n for n in exported if "train" in n) == TRAIN_ENTRIES
    assert sorted(n for n, _, _ in L.SIGNATURES if "train" in n) == TRAIN_ENTRIES
    assert not [n for n in exported if "_wg" in n or "any_chain" in n]


def problem():
    rng = np.random.default_rng(11)
    specs = [O.LayerSpec(2, 4, 5, "tanh_fast"), O.LayerSpec(4, 2, 5, "tanh_fast")]   # a pruned LV net
    p = torch.as_tensor(rng.uniform(-0.3, 0.3, 96))
    u0 = torch.as_tensor(rng.uniform(0.5, 2.0, (1, 2)))
    X = torch.as_tensor(rng.uniform(0.5, 2.0, (35, 1, 2)))
    return OracleChainRHS(specs), u0, X, p


def test_bad_device_loop_raises():
    rhs, u0, X, p = problem()
    ts = [0.1 * i for i in range(35)]
    for bad in ("all", "", None, 1):
        with pytest.raises(ValueError, match="device_loop"):
            kanode.Trainer(rhs, u0, (0.0, 3.5), ts, X, p, device_loop=bad)
    assert kanode.Trainer(rhs, u0, (0.0, 3.5), ts, X, p).device_loop == "default"


def test_device_loop_any_without_a_gpu_is_the_host_loop():
    """On the CPU "any" changes nothing: run() is the loop of step() calls, bit for bit."""
    rhs, u0, X, p = problem()
    ts = [0.1 * i for i in range(35)]
    a = kanode.Trainer(rhs, u0, (0.0, 3.5), ts, X, p, eta=1e-3, device_loop="any")
    b = kanode.Trainer(rhs, u0, (0.0, 3.5), ts, X, p, eta=1e-3)
    out = a.run(2)
    ls = [b.step(), b.step()]
    assert a.last_run == "host"
    assert torch.equal(a.p, b.p) and out["loss"].tolist() == ls == a.history
