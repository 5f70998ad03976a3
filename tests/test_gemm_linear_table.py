"""The route table of tests/gemm_linear_child.py, checked on the CPU: a plain-Python transcription of the conditions of dispatch_gemm,
plan_splitk (csrc/gemm.hip), launch_gemm_pipe (csrc/gemm_pipe.hip) and gemm_small_applies (csrc/gemm_small.hip), for the launches the
child makes, must give the hand-written route of every (case, switch set); and the table must reach every family with a ragged-M
case, a ragged-N case and every epilogue form the family accepts."""
from collections import defaultdict

from tests.gemm_linear_child import CASES, SWITCHES, expected_route, names_of

WS_BYTES = 32 << 20   # the scratch the stand-alone op wrappers hand over (paddlemix_amd/ops.py _workspace)
CUS = 256


def _pick_model(M, N):
    """pick_tile_model for a plain launch of at most 256 tiles of 128 x 128 (every unforced case): one round of each candidate"""
    assert -(-M // 128) * -(-N // 128) <= CUS
    if M < 256:
        return 128
    cost = {128: 256 * 0.95, 160: 416 * 0.6, 257: 512, 320: 576}   # (bm + bn, the weights of the 128 and the 256 x 160 tile)
    return min(cost, key=cost.get)


def model_route(name, sw):
    M, N, K, kind = CASES[name][:4]
    env = SWITCHES[sw]
    kind = kind.split(":")[0]
    f8, ln, geglu, a_rpb = kind.startswith("f8"), kind.startswith("ln"), kind.endswith("geglu"), kind == "a-remap"
    nt = -(-K // 64)
    forced = int(env.get("MI355X_SD_GEMM_TILE", 0))
    tile = forced or _pick_model(M, N)
    if not forced and tile == 128:   # gemm_small_applies (every case: M <= 4096, <= 128 tiles of 128 x 128)
        assert M <= 4096 and -(-M // 128) * -(-N // 128) <= 128
        if not f8 and K % 64 == 0 and nt <= 48:
            return "small"
    splitk = 0
    if tile == 128 and "MI355X_SD_NO_SPLITK" not in env:   # plan_splitk
        tiles = -(-M // 128) * -(-N // 128)
        if tiles <= 160 and nt >= 8:
            s = min(-(-416 // tiles), nt // 4, WS_BYTES // (M * N * 4))
            if s >= 2:
                kc = -(-nt // s)
                splitk = -(-nt // kc)
                splitk = splitk if splitk >= 2 else 0
    sk = "+splitk" if splitk else ""
    pipe_ok = ("MI355X_SD_NO_PIPE" not in env and not f8 and K % 64 == 0 and not (tile == 160 and geglu)
               and tile in (128, 160, 320, 256, 129) and not (geglu and tile == 129) and not (tile == 129 and ln))
    if pipe_ok:
        return f"pipe/{tile}{sk}"
    if ln:
        if tile == 257 and K % 64 == 0:
            return "gemm256+ln"
        t = 256 if tile in (256, 257) else 160 if tile == 160 and not geglu else 320 if tile == 320 else 128
        return f"generic/{t}+ln{sk}"
    if f8:
        assert K % 16 == 0
        t = 160 if tile == 160 and not geglu else 320 if tile == 320 else 256 if tile in (256, 257) else 128
        return f"generic/{t}+f8{sk}"
    if tile == 257 and K % 64 == 0 and not a_rpb:
        return "gemm256"
    t = 256 if tile in (256, 257) else 160 if tile == 160 and not geglu else 320 if tile == 320 else 128
    return f"generic/{t}{sk}"


def test_the_table_is_what_the_dispatch_conditions_give():
    for sw in SWITCHES:
        for name in names_of(sw):
            assert expected_route(name, sw) == model_route(name, sw), (sw, name)


def test_persistent_cases_exceed_the_grid_cap_by_a_few_tiles():
    for t, (bm, bn, cap) in {"128": (128, 128, 2 * CUS), "129": (128, 160, 2 * CUS), "160": (256, 160, CUS), "320": (256, 320, CUS),
                             "256": (256, 256, CUS)}.items():
        M, N = CASES[f"persist {t}"][:2]
        tiles = -(-M // bm) * -(-N // bn)
        assert cap < tiles <= cap + 32, (t, tiles)


BM = {"generic/128": 128, "generic/160": 256, "generic/256": 256, "generic/320": 256, "pipe/128": 128, "pipe/129": 128, "pipe/160": 256,
      "pipe/320": 256, "pipe/256": 256, "gemm256": 256, "small": 64}
BN = {"generic/128": 128, "generic/160": 160, "generic/256": 256, "generic/320": 320, "pipe/128": 128, "pipe/129": 160, "pipe/160": 160,
      "pipe/320": 320, "pipe/256": 256, "gemm256": 256, "small": 64}
K16 = {"plain", "nobias", "scale", "silu", "gelu", "geglu", "R", "R-nobias", "Rwide", "R32", "rowbias", "rowbias+R", "rowbias+R32",
       "gate+R", "a-remap", "c-remap", "strided"}
KLN = {"ln", "ln-nobias", "ln-geglu"}
KF8 = {"f8", "f8-nobias", "f8-gelu", "f8-gate+R"}


def test_every_family_has_ragged_edges_and_every_epilogue_form_it_accepts():
    reach = defaultdict(list)
    for sw in SWITCHES:
        for name in names_of(sw):
            reach[expected_route(name, sw)].append(name)
    for fam, names in reach.items():
        base = fam.split("+")[0]
        assert any(CASES[n][0] % BM[base] for n in names), ("ragged M", fam)
        assert any(CASES[n][1] % BN[base] for n in names), ("ragged N", fam)
        kinds = {CASES[n][3].split(":")[0] for n in names}
        if "+splitk" in fam:   # (the form is the reduce kernel's: the shared epilogue, reached with a residual, the fold and the scale)
            continue
        if "+ln" in fam:
            want = KLN - ({"ln-geglu"} if base == "generic/160" else set())
        elif "+f8" in fam:
            want = KF8
        else:
            want = K16 - ({"geglu"} if base.endswith(("/160", "/129")) else set()) - ({"a-remap"} if base == "gemm256" else set())
            if base.startswith("pipe") or base == "small":   # (LN launches of these families carry no +ln in the route)
                want = want | (KLN if base != "pipe/129" else set()) - ({"ln-geglu"} if base == "pipe/160" else set())
        assert want <= kinds, (fam, sorted(want - kinds))
