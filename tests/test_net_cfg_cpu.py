"""What a handle is, host side (no GPU): the parameter table of every kind of network and the message of every refused
configuration, against the record in tests/golden/net_cfg_baseline.json (tools/table_identity.py --out writes it).

The tables are part of the ABI: dsd_param_info indices, and the declaration order the one GEMM over all emb_layers takes its
columns from.  The messages are what dsd_create / dsd_create_disc / dsd_block_create answer; three cases pin the order in which
the rules of one handle are checked."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import table_identity  # noqa: E402

BASE = json.load(open(os.path.join(ROOT, "tests", "golden", "net_cfg_baseline.json")))


@pytest.fixture(scope="module")
def got():
    tables, errors, _ = table_identity.collect()
    return {"tables": tables, "errors": errors}


def test_the_record_covers_every_kind_and_rule():
    assert len(BASE["tables"]) == 30 and sum(len(t) for t in BASE["tables"].values()) == 2719
    assert len(BASE["errors"]) == 76
    kinds = {m.split(" needs ")[0] for m in BASE["errors"].values() if m.startswith("block kind ")}
    assert kinds == {f"block kind {k}" for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 14)}        # the eleven kinds with a fixed argument count
    for text in ("DiT handle needs", "DiT: unsupported geometry", "DiT: bad configuration", "VAE handle needs", "VAE: bad ch_mult",
                 "VAE: bad attn_resolutions", "VAE: ch = ", "VAE: bad configuration", "UNetModel handle needs", "UNetModel: bad channel_mult",
                 "UNetModel: bad attention_resolutions", "UNetModel: spatial transformer needs", "UNetModel: label_emb kind 4",
                 "needs a width", "unknown block kind", "UNet_disc_Model: channel_mult[0]"):
        assert any(text in m for m in BASE["errors"].values()), text


@pytest.mark.parametrize("name", sorted(BASE["tables"]))
def test_parameter_table_equals_the_record(got, name):
    assert got["tables"][name] == BASE["tables"][name]


def test_every_refusal_equals_the_record_character_by_character(got):
    assert sorted(got["errors"]) == sorted(BASE["errors"])
    different = {k: (got["errors"][k], v) for k, v in BASE["errors"].items() if got["errors"][k] != v}
    assert not different
