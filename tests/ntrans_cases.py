"""Case lists shared by tests/test_ntrans_cpu.py, tests/test_ntrans_gpu.py and tools/make_golden_ntrans.py: the batched Nystrom
stages, the whole batched attention, the b = 1 bit-identity lengths, the two encoder modes (attn='ntrans' /
region_attn='ntrans') and RRTMIL around them.  Every input and parameter regenerates from rrt_mil_amd.synth."""
import math

import numpy as np

from rrt_mil_amd import synth

DIM, HEADS = 128, 2
PINV_ITERATIONS = 6
PEAK = 6.0                   # the peaked case: item 1's logits are this many times the other items'

# name -> (b, n, peaked) and what a kernel can get wrong there; np = n rounded up to 256
STAGE_CASES = {
    "b3_n144": (3, 144, False),          # l = 1, 112 zero rows in FRONT of every item: a neighbour's rows behind them
    "b3_n300": (3, 300, False),          # l = 2, 212 pad rows: half-pad landmarks, two key sub-chunk pairs, eight token tiles
    "b3_n256": (3, 256, False),          # no pad: the stencil's window ends exactly where the next item begins
    "b3_n144_peaked": (3, 144, True),    # one item's column sums far above the others': the scale is ONE scalar
}
ATTN_CASES = dict(STAGE_CASES, b16_n16=(16, 16, False))      # many short items: 240 all-zero landmarks each
BIT_IDENTITY_LENGTHS = (300, 1000)
STAGES = ("landmarks", "landmark_sim", "landmark_attn", "pinv", "zav", "output")


def batch_inputs(b, n, peaked, dim=DIM, heads=HEADS):
    """(NystromAttention state_dict as numpy, x [b, n, dim])"""
    state = synth.nystrom_state(dim, heads, gain=1.0, tag="ntrans")
    x = np.stack([synth.nystrom_input(n, dim, tag=f"ntrans/item{i}") for i in range(b)])
    if peaked:
        x[1] *= np.float32(math.sqrt(PEAK))      # logits are quadratic in the rows
    return state, x


# the encoder: RRTEncoder(mlp_dim=128, n_heads=2, crmsa_heads=2, **cfg) on a bag of N tokens
ENC_BASE = dict(mlp_dim=128, n_heads=2, crmsa_heads=2)
ENCODER_CASES = {
    "bag_n300": (dict(attn="ntrans"), 300),
    "bag_n700_l3_ffn_sc": (dict(attn="ntrans", n_layers=3, ffn=True, all_shortcut=True), 700),
    "reg_n200_rn2": (dict(region_attn="ntrans", region_num=2), 200),                          # P = 64, R = 4, np = 256
    "reg_n1300_rn2_sc": (dict(region_attn="ntrans", region_num=2, all_shortcut=True), 1300),   # P = 361, np = 512
    "reg_n1000_rn4": (dict(region_attn="ntrans", region_num=4), 1000),                         # R = 16
    "reg_n500_rsize9": (dict(region_attn="ntrans", region_size=9), 500),                       # H = 27: R = 9, P = 81
    "reg_n300_fallback": (dict(region_attn="ntrans", region_num=8, min_region_ratio=2.0), 300),   # 276 > 300 / 2: one region of 324
    "bag_n300_ppeg_first": (dict(attn="ntrans", pos="ppeg", pos_pos=-1), 300),                  # PPEG in front of layer 0
    "reg_n200_l3_peg_mid": (dict(region_attn="ntrans", region_num=2, n_layers=3, pos="peg", pos_pos=0), 200),   # PEG before layer 1
}
GOLDEN_ROWS = 4              # rows 0, 1, N // 2, N - 1 of the reference's float64 output

MIL_N, MIL_INPUT_DIM = 200, 1024
MIL_CASES = {
    "mil_regions_rn2": dict(region_attn="ntrans", region_num=2),
    "mil_bag": dict(attn="ntrans"),
}


def golden_rows(N):
    return [0, 1, N // 2, N - 1]


def is_bag(cfg):
    return cfg.get("attn") == "ntrans"


def ntrans_state(cfg, prefix=""):
    """synth.encoder_state's parameters with the R-MSA layers' attention replaced by NystromAttention's four tensors, under the
    reference's keys: layers.i.attn.* (attn='ntrans') or layers.i.attn.attn.* (region_attn='ntrans')"""
    kw = {k: v for k, v in cfg.items() if k not in ("attn", "region_attn")}
    base = synth.encoder_state(epeg=False, **kw)
    dim, heads = kw.get("mlp_dim", 512), kw.get("n_heads", 8)
    out = {}
    for k, v in base.items():
        if k.startswith("layers.") and ".attn.attn." in k:
            continue
        out[prefix + k] = v
    for i in range(kw.get("n_layers", 2) - 1):
        sub = f"layers.{i}.attn." + ("" if is_bag(cfg) else "attn.")
        for k, v in synth.nystrom_state(dim, heads, gain=1.0, tag=f"ntrans/layer{i}").items():
            out[prefix + sub + k] = v
    return out


def encoder_inputs(name):
    """(constructor arguments, state_dict as numpy, bag [N, 128])"""
    extra, N = ENCODER_CASES[name]
    cfg = dict(ENC_BASE, **extra)
    return cfg, ntrans_state(cfg), synth.bag(N, cfg["mlp_dim"], tag="ntrans")


def mil_inputs(name):
    """(RRTMIL constructor arguments, state_dict as numpy, features [200, 1024])"""
    cfg = dict(MIL_CASES[name])
    state = {k: v for k, v in synth.mil_state(input_dim=MIL_INPUT_DIM, epeg=False).items() if not k.startswith("online_encoder.")}
    state.update(ntrans_state(dict(cfg, mlp_dim=512, n_heads=8), prefix="online_encoder."))
    return cfg, state, synth.bag(MIL_N, MIL_INPUT_DIM, tag="ntrans_mil")
