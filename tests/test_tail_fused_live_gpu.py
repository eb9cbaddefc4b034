"""The fused up-sampler tail computes GEMM 1 over each wave's 85 live u1 pixels only (three fragments instead of four).

GPU: every entry point of tail_fused.hip (fcvsr_tail_fused, _base, _u8, _u16, _base_u8, _base_u16; both quantisations of the integer
ones) gives the bytes the kernel gave before that change: tests/golden/tail_fused_parent_hashes.json holds the sha256 of each result
as computed on an MI355X by the library built from the commit before it (scripts/record_tail_fused_hashes.py, which runs
`result_hashes` below with whatever library is in the tree).  Both 16-bit dtypes, one slope inside [0, 1] (PReLU as max(x, s*x)) and
one outside (the generic form is a separate tile loop).  Shapes (centre LR frame h x w; u1 is 2h x 2w, the result 4h x 4w), B = 2:
    1 x 1     4 x 4 result: all four borders inside one tile
    2 x 8     8 x 32: exactly one full tile
    3 x 9     12 x 36: 2 x 2 tiles, the last row / column of tiles four rows / four columns wide
    5 x 17    20 x 68: 3 x 3 tiles, one of them fully interior (no padding pass)
and B = 32 of 8 x 64: 1024 tiles, more than the workgroups any device launches (three per CU), so a workgroup walks a run of
several tiles across an image boundary.

CPU: the (p, sy, sx) -> (hr, hc) map of the kernel, restated here, sends the four waves' 85 live pixels to each of the 340 halo
positions exactly once, and every surplus slot of the last fragment is dead."""
import ctypes as C
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tail_fused_parent_hashes.json")

SHAPES = [(2, 1, 1), (2, 2, 8), (2, 3, 9), (2, 5, 17), (32, 8, 64)]          # (B, h, w) of the centre LR frame
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}
SLOPES = [0.25, 1.5]
GROUPS = [(shape, dn, slope) for shape in SHAPES for dn in DTYPES for slope in SLOPES]


# ---- the kernel's pixel map, restated ------------------------------------------------------------------------------------------
TH, TW = 8, 32                                               # output tile
HH, HW = TH + 2, TW + 2                                      # its halo: 10 x 34
UH, UW = TH // 2 + 2, TW // 2 + 2                            # u1 pixels under the halo: 6 x 18
LH, LW = UH - 1, UW - 1                                      # a wave's live pixels: 5 x 17
NL, NF = LH * LW, (LH * LW + 31) // 32                       # 85 pixels in 3 fragments of 32 slots


def _slot(p, sy, sx):
    """Slot p of wave (sy, sx): (uy, ux) of the u1 pixel it loads and the halo position it stores to (None: dead slot)."""
    live = p < NL
    q = min(p, NL - 1)                                       # surplus slots load the last live pixel
    uy, ux = 1 - sy + q // LW, 1 - sx + q % LW
    hr, hc = 2 * uy + sy - 1, 2 * ux + sx - 1
    return (uy, ux), ((hr, hc) if live else None)


def test_live_pixels_cover_the_halo_exactly_once():
    assert (NL, NF) == (85, 3)
    hits = np.zeros((HH, HW), np.int64)
    for sy in range(2):
        for sx in range(2):
            seen = set()
            for p in range(NF * 32):
                (uy, ux), dst = _slot(p, sy, sx)
                assert 0 <= uy < UH and 0 <= ux < UW, "every slot, dead ones included, loads one of the tile's 6 x 18 u1 pixels"
                if p >= NL:
                    assert dst is None, f"surplus slot {p} of wave ({sy}, {sx}) is not dead"
                    continue
                hr, hc = dst
                assert 0 <= hr < HH and 0 <= hc < HW, f"live slot {p} of wave ({sy}, {sx}) leaves the halo: {dst}"
                assert (hr % 2, hc % 2) == ((sy + 1) % 2, (sx + 1) % 2)      # halo (0, 0) is output pixel (-1, -1)
                assert (uy, ux) not in seen
                seen.add((uy, ux))
                hits[hr, hc] += 1
            assert len(seen) == NL
            assert NF * 32 - NL == 11
    assert hits.sum() == HH * HW == 340 and (hits == 1).all(), "each halo position is produced exactly once"


def test_dropped_pixels_are_the_ones_that_missed_the_halo():
    """The 23 u1 pixels a wave no longer multiplies are exactly those whose sub-pixel fell outside the 10 x 34 halo."""
    for sy in range(2):
        for sx in range(2):
            live = {_slot(p, sy, sx)[0] for p in range(NL)}
            for uy in range(UH):
                for ux in range(UW):
                    hr, hc = 2 * uy + sy - 1, 2 * ux + sx - 1
                    assert ((uy, ux) in live) == (0 <= hr < HH and 0 <= hc < HW)


# ---- bit-equality with the kernel before the change ---------------------------------------------------------------------------
def _dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda().view(torch.uint16)


@functools.lru_cache(maxsize=2)
def _problem(B, h, w, dn, slope):
    from fcvsr_amd import hip
    dt = DTYPES[dn]
    rs = np.random.RandomState(1000 * h + w + (7 if dn == "f16" else 0) + int(slope * 100))
    f32 = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))
    p = {}
    p["u1"] = f32(B, 2 * h, 2 * w, 64).to(dt).cuda()
    w2, b2, wl = f32(256, 64, 1, 1) / 8, f32(256) * 0.1, f32(1, 64, 3, 3) / 240
    p["w2"] = hip.pack_conv_weight_mfma(w2.cuda(), dt, ps=True)
    p["b2"] = b2[hip.ps_order(256)].contiguous().cuda()
    tab = torch.zeros(16, 64)
    tab[:9] = wl[0].permute(1, 2, 0).reshape(9, 64)
    p["wl"] = tab.to(dt).contiguous().cuda()
    p["bl"] = torch.tensor([0.03]).cuda()
    p["slope"] = torch.tensor([slope]).cuda()
    # the centre frame as the engine passes it: a strided (B,h,w,1) view into the (B,T,1,h,w) window
    f8 = rs.randint(0, 256, (B, 7, 1, h, w)).astype(np.uint8)
    f16 = rs.randint(0, 1100, (B, 7, 1, h, w)).astype(np.uint16)           # some samples above 1023
    p["c8"] = torch.from_numpy(f8).cuda()[:, 3].permute(0, 2, 3, 1)
    p["c16"] = _dev16(f16)[:, 3].permute(0, 2, 3, 1)
    p["cf"] = (torch.from_numpy(f8).float() / 255).cuda()[:, 3].permute(0, 2, 3, 1)
    p["base"] = torch.from_numpy(rs.uniform(0.2, 0.8, (B, 1, 4 * h, 4 * w)).astype(np.float32)).cuda()
    return p


def _sha(t):
    if t.dtype == torch.uint16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def result_hashes(B, h, w, dn, slope):
    """{case name: sha256 of the result} of every entry point of tail_fused.hip on one problem, with the library in the tree."""
    from fcvsr_amd import hip
    L, st = hip.lib(), hip.stream_ptr()
    p = _problem(B, h, w, dn, slope)
    wa = (p["w2"].data_ptr(), p["b2"].data_ptr(), p["slope"].data_ptr(), p["wl"].data_ptr(), p["bl"].data_ptr())
    u1v, bv = hip.view(p["u1"]), hip.view(p["base"].permute(0, 2, 3, 1))
    dims = (B, 2 * h, 2 * w)
    tag = f"{dn}/B{B}_{h}x{w}/slope{slope}"
    out = {}

    def result(dtype, fill):
        if dtype == torch.uint16:
            t = torch.empty(B, 1, 4 * h, 4 * w, device="cuda", dtype=torch.int16).fill_(fill).view(torch.uint16)
        else:
            t = torch.full((B, 1, 4 * h, 4 * w), fill, device="cuda", dtype=dtype)
        return t, hip.view(t.permute(0, 2, 3, 1))

    got = p["base"].clone()                                  # read-modify-write: out holds the base skip
    hip.check(L.fcvsr_tail_fused(C.byref(u1v), *wa, *dims, C.byref(hip.view(got.permute(0, 2, 3, 1))), st), "fcvsr_tail_fused")
    assert torch.isfinite(got).all() and float((got - p["base"]).abs().max()) > 0.01          # the tail term is really there
    out[f"fcvsr_tail_fused/{tag}"] = _sha(got)
    got, gv = result(torch.float32, float("nan"))            # write-only: whatever it held must not matter
    cv = hip.view(p["cf"])
    hip.check(L.fcvsr_tail_fused_base(C.byref(u1v), *wa, C.byref(cv), *dims, C.byref(gv), st), "fcvsr_tail_fused_base")
    assert torch.isfinite(got).all()
    out[f"fcvsr_tail_fused_base/{tag}"] = _sha(got)
    for qn, q in hip.QUANTISE.items():
        for sfx, dtype, centre, table in (("u8", torch.uint8, p["c8"], hip.u8_table("cuda")),
                                          ("u16", torch.uint16, p["c16"], hip.u16_table("cuda"))):
            got, gv = result(dtype, 77)
            hip.check(getattr(L, f"fcvsr_tail_fused_{sfx}")(C.byref(u1v), *wa, *dims, C.byref(bv), C.byref(gv), q, st),
                      f"fcvsr_tail_fused_{sfx}")
            out[f"fcvsr_tail_fused_{sfx}/{qn}/{tag}"] = _sha(got)
            got, gv = result(dtype, 77)
            cv = hip.view(centre)
            hip.check(getattr(L, f"fcvsr_tail_fused_base_{sfx}")(C.byref(u1v), *wa, C.byref(cv), table.data_ptr(), *dims, C.byref(gv),
                                                                 q, st), f"fcvsr_tail_fused_base_{sfx}")
            out[f"fcvsr_tail_fused_base_{sfx}/{qn}/{tag}"] = _sha(got)
    torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dn,slope", GROUPS, ids=[f"B{s[0]}_{s[1]}x{s[2]}-{d}-slope{sl}" for s, d, sl in GROUPS])
def test_every_entry_point_gives_the_parent_commits_bytes(shape, dn, slope):
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"]
    got = result_hashes(*shape, dn, slope)
    assert len(got) == 10                                    # 2 f32 entry points + 4 integer ones x 2 quantisations
    missing = sorted(k for k in got if k not in want)
    assert not missing, f"not recorded in {os.path.basename(GOLDEN)}: {missing}"
    diff = sorted(k for k in got if got[k] != want[k])
    assert not diff, f"{len(diff)} of {len(got)} results differ from the recorded bytes: {diff}"


def test_golden_file_lists_exactly_the_cases_of_this_file():
    with open(GOLDEN) as f:
        want = json.load(f)["sha256"]
    names = set()
    for (B, h, w), dn, slope in GROUPS:
        tag = f"{dn}/B{B}_{h}x{w}/slope{slope}"
        names |= {f"fcvsr_tail_fused/{tag}", f"fcvsr_tail_fused_base/{tag}"}
        names |= {f"fcvsr_tail_fused{b}_{s}/{q}/{tag}" for b in ("", "_base") for s in ("u8", "u16") for q in ("truncate", "round")}
    assert set(want) == names and len(names) == 200
    assert len(set(want.values())) == len(want), "two cases with the same bytes: a result that ignores its inputs"
