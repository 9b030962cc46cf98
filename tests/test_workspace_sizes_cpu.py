"""Every workspace size the library reports, over a grid of bag sizes and configurations, against the recorded table
tests/golden/workspace_sizes.json (CPU: the size queries launch nothing).

A workspace layout is stated once in csrc/api.hip -- one carve function serves the size query and the real carve -- and
callers size their buffers by these numbers, so a refactor of the carving must return them byte for byte.  The table was
recorded from the library before the carves moved to the shared arena; `python tests/test_workspace_sizes_cpu.py FILE`
writes the current library's table to FILE.
"""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:        # (run as a script, to write a table: no conftest has done it)
    sys.path.insert(0, ROOT)

from rrt_mil_amd import _lib  # noqa: E402

GOLDEN =os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "workspace_sizes.json")
NS = (1, 33, 300, 9000, 30000)
ENCODERS = {
    "default": {},
    "ffn": dict(ffn=1),
    "crmsa_mlp": dict(crmsa_mlp=1),
    "ppeg": dict(pos=_lib.POS_PPEG, pos_pos=-1),
    "peg_l3": dict(pos=_lib.POS_PEG, pos_pos=0, n_rmsa_layers=2),
    "l3": dict(n_rmsa_layers=2),
    "no_crmsa": dict(cr_msa=0),
    "crmsa_only": dict(n_rmsa_layers=0),
    "value_bf": dict(epeg_type=_lib.EPEG_VALUE_BF),
    "attn2d": dict(epeg_2d=1, epeg_k=9),
    "r16_k5_d256": dict(dim=256, region_num=16, crmsa_k=5, ffn_hidden=1024),
}


def encoder_desc(**kw):
    f = dict(dim=512, n_heads=8, n_rmsa_layers=1, region_num=8, epeg=1, epeg_k=15, cr_msa=1, crmsa_k=3, crmsa_heads=8,
             ffn_act=_lib.ACT_GELU, ffn_hidden=2048, peg_k=7)
    f.update(kw)
    return _lib.EncoderDesc(**f)


def _head_desc(cls, enc, **kw):
    d = cls()
    if enc is not None:
        C.memmove(C.byref(d.enc), C.byref(encoder_desc(**ENCODERS[enc])), C.sizeof(_lib.EncoderDesc))
    else:
        d.enc.dim = 512
    if hasattr(d, "has_rrt"):
        d.has_rrt = int(enc is not None)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def size_table(lib):
    """{case: [return code, bytes...]} of every *_workspace_size / *_sizes entry point over the grid"""
    t = {}

    def q(key, fn, *args, outs=1):
        b = [C.c_size_t(0) for _ in range(outs)]
        rc = fn(*args, *[C.byref(v) for v in b])
        t[key] = [rc] + [v.value for v in b]

    for n in NS:
        for name, kw in ENCODERS.items():
            d = encoder_desc(**kw)
            q(f"encoder/{name}/n{n}", lib.rrt_encoder_workspace_size, C.byref(d), n)
            for batch in (1, 3):
                q(f"encoder_batch/{name}/b{batch}/n{n}", lib.rrt_encoder_batch_workspace_size, C.byref(d), batch, n)
            q(f"encoder_train/{name}/n{n}", lib.rrt_encoder_train_sizes, C.byref(d), n, outs=2)
        for gated in (0, 1):
            q(f"pool/gated{gated}/n{n}", lib.rrt_pool_workspace_size, n, 512, 128, gated)
        q(f"attn_pool/n{n}", lib.rrt_attn_pool_workspace_size, n, 512, 128)
        for k in (1, 8):
            for hidden in (256, 384):
                q(f"branch_pool/h{hidden}/k{k}/n{n}", lib.rrt_branch_pool_workspace_size, n, 512, hidden, k)
            q(f"instance_max/k{k}/n{n}", lib.rrt_instance_max_workspace_size, n, 512, k)
            q(f"dsmil_pool/k{k}/n{n}", lib.rrt_dsmil_pool_workspace_size, n, 512, 128, k)
        for enc in list(ENCODERS) + [None]:
            if enc == "r16_k5_d256":            # (the heads are 512 wide)
                continue
            for in_dim in (1024, 96):
                if enc is not None:
                    for gated in (0, 1):
                        d = _head_desc(_lib.MilDesc, enc, input_dim=in_dim, emb_act=_lib.ACT_RELU, n_classes=2, pool_hidden=128,
                                       pool_act=_lib.ACT_RELU, pool_gated=gated)
                        q(f"mil/{enc}/in{in_dim}/gated{gated}/n{n}", lib.rrt_mil_workspace_size, C.byref(d), n)
                for k in (1, 8):
                    for gated in (0, 1):
                        d = _head_desc(_lib.ClamDesc, enc, input_dim=in_dim, emb_act=_lib.ACT_RELU, n_classes=max(k, 2),
                                       per_branch=int(k > 1), gated=gated, hidden=256 if gated else 384, k_sample=8)
                        q(f"clam/{enc}/in{in_dim}/gated{gated}/k{k}/n{n}", lib.rrt_clam_workspace_size, C.byref(d), n)
                    d = _head_desc(_lib.DsmilDesc, enc, input_dim=in_dim, emb_act=_lib.ACT_RELU, n_classes=k, q_dim=128)
                    q(f"dsmil/{enc}/in{in_dim}/k{k}/n{n}", lib.rrt_dsmil_workspace_size, C.byref(d), n)
        for heads in (8, 4):
            nd = _lib.NystromDesc(dim=512, heads=heads, dim_head=64, num_landmarks=256, pinv_iterations=6, residual=1,
                                  residual_conv_kernel=33)
            q(f"nystrom/h{heads}/n{n}", lib.rrt_nystrom_workspace_size, C.byref(nd), n)
            td = _lib.TransmilDesc(input_dim=1024, n_classes=2, act=_lib.ACT_RELU, attn=nd)
            q(f"transmil/h{heads}/n{n}", lib.rrt_transmil_workspace_size, C.byref(td), n)
    return t


@pytest.fixture(scope="module")
def tables():
    with open(GOLDEN) as fh:
        return json.load(fh), size_table(_lib.load())


def test_grid_is_the_recorded_one(tables):
    want, got = tables
    assert sorted(got) == sorted(want)


def test_every_size_query_succeeds_somewhere(tables):
    """the table is not a list of refusals: every entry point reports a size at every N for some configuration"""
    want, _ = tables
    ok = {(k.split("/")[0], k.rsplit("/", 1)[1]) for k, v in want.items() if v[0] == 0 and all(b > 0 for b in v[1:])}
    assert ok == {(k.split("/")[0], k.rsplit("/", 1)[1]) for k in want}


def test_workspace_sizes_equal_the_table(tables):
    want, got = tables
    bad = {k: (want[k], got[k]) for k in want if got.get(k) != want[k]}
    assert not bad, f"{len(bad)} of {len(want)} sizes differ, e.g. {sorted(bad.items())[:5]}"


if __name__ == "__main__":
    with open(sys.argv[1], "w") as out:
        json.dump(size_table(_lib.load(os.environ.get("RRT_HIP_LIB"))), out, indent=0, sort_keys=True)
        out.write("\n")
