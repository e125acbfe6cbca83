"""The capacity protocol's host arithmetic, without a GPU: the library's direct-bins decision (api.hip slam_direct_bins, exported as
mm3dgs_slam_direct_bins) against the rule it had while it still carried the record capacity of the Gaussian-major block records, and
FusedEngine.sizing against the capacities the engine picked then."""
from mm3dgs_slam_amd import _lib
from mm3dgs_slam_amd.fused import FusedEngine

ALL = _lib.FWD_STATE_CLEAN | _lib.FWD_SHORT_LISTS | _lib.FWD_DIRECT_BINS
CLAUSES = ("clean", "short", "direct", "slot_bits", "tiles", "bin_cap", "trec_cap", "4P")


def _old_rule(P, N, flags, H, W):
    """The decision as it stood with the clause on the block-record capacity (16 N / nb, at least 1024): (the kept clauses by name, the dropped clause)."""
    T = ((W + 15) // 16) * ((H + 15) // 16)
    nb = max((P + 255) // 256, 1)
    idb = 1
    while idb < 31 and (1 << idb) < P:
        idb += 1
    slot_bits = min(32 - idb, 13)
    bin_cap = min(N // max(T, 1), (1 << max(slot_bits, 1)) - 1)
    records = min(16 * N // nb, 0xffffffff // nb)      # block records per projection workgroup
    trec_cap = min(N // nb, 0xffffffff // nb)
    kept = {"clean": bool(flags & _lib.FWD_STATE_CLEAN), "short": bool(flags & _lib.FWD_SHORT_LISTS), "direct": bool(flags & _lib.FWD_DIRECT_BINS),
            "slot_bits": slot_bits >= 10, "tiles": T <= 11264 and T <= 12288, "bin_cap": bin_cap >= 32, "trec_cap": trec_cap >= 256, "4P": N >= 4 * P}
    return kept, records >= 1024


def test_direct_bins_decision_is_what_it_was_with_the_record_capacity_clause(monkeypatch):
    """The dropped clause, records >= 1024, followed from the clauses that stay (trec_cap >= 256: N / nb >= 256 and 0xffffffff / nb >= 256; slot_bits >= 10: P <= 2^22,
    nb <= 2^14, 0xffffffff / nb >= 2^18; floor(16 N / nb) >= 16 floor(N / nb) >= 4096): over the boundaries of every clause the library answers as
    the old rule does, every kept clause decides a case on its own, and the dropped one never does."""
    for name in ("MM3DGS_NO_DIRECT_BINS", "MM3DGS_NO_FUSED_SCAN", "MM3DGS_NO_FUSED_SORT", "MM3DGS_DIRECT_MAX_TILES"):
        monkeypatch.delenv(name, raising=False)
    lib = _lib.load()
    sole, ones, rec_false = set(), 0, 0
    # (16x16 and 2160x3840 beside the three SLAM sizes: one tile, where trec_cap alone can decide, and a grid beyond the binning kernel's LDS)
    for H, W in ((16, 16), (48, 64), (480, 640), (1080, 1920), (2160, 3840)):
        cam = _lib.Mm3dgsCamera()
        cam.image_height, cam.image_width, cam.tanfovx, cam.tanfovy = H, W, 0.6, 0.45
        T = ((W + 15) // 16) * ((H + 15) // 16)
        for P in (1, 256, 257, 1 << 19, (1 << 19) + 1, 1 << 22, (1 << 22) + 1):
            nb = (P + 255) // 256
            edges = (4 * P, 256 * nb, 32 * T)
            for N in sorted({e - 1 for e in edges} | set(edges) | {max(edges), 1 << 31}):
                for flags in (ALL, ALL & ~_lib.FWD_STATE_CLEAN, ALL & ~_lib.FWD_SHORT_LISTS, ALL & ~_lib.FWD_DIRECT_BINS):
                    kept, rec = _old_rule(P, N, flags, H, W)
                    want = int(all(kept.values()) and rec)
                    assert lib.mm3dgs_slam_direct_bins(cam, P, N, flags) == want, (H, W, P, N, flags, kept, rec)
                    ones += want
                    failing = [k for k, v in kept.items() if not v]
                    if len(failing) == 1:
                        sole.add(failing[0])
                    rec_false += not rec
                    assert rec or not (kept["trec_cap"] and kept["slot_bits"]), (H, W, P, N)
    assert sole == set(CLAUSES), sole
    assert ones >= 40 and rec_false >= 40, (ones, rec_false)


# (P, ratio, max_tile_len, H, W, want, direct): what _ensure computed for these inputs while it still read the header's record maximum, which
# the device never wrote (0): ratio None (nothing measured), a tiny ratio at a million Gaussians (the 64-pairs-per-workgroup floor binds at
# 48x64), lists either side of FAST_PATH_MAX_LIST, maps either side of the slot-bit limits, P = 0 and 1
SIZING = (
    (0, None, 1073741824, 480, 640, 65584, False),
    (0, None, 700, 480, 640, 65584, False),
    (0, None, 2048, 480, 640, 65584, False),
    (0, None, 2049, 480, 640, 65584, False),
    (0, 0.01, 1073741824, 480, 640, 65536, False),
    (0, 0.01, 700, 480, 640, 65536, False),
    (0, 0.01, 2048, 480, 640, 65536, False),
    (0, 0.01, 2049, 480, 640, 65536, False),
    (0, 2.3, 1073741824, 480, 640, 65540, False),
    (0, 2.3, 700, 480, 640, 65540, False),
    (0, 2.3, 2048, 480, 640, 65540, False),
    (0, 2.3, 2049, 480, 640, 65540, False),
    (1, None, 1073741824, 480, 640, 65584, False),
    (1, None, 700, 480, 640, 1413600, True),
    (1, None, 2048, 480, 640, 3840000, True),
    (1, None, 2049, 480, 640, 65584, False),
    (1, 0.01, 1073741824, 480, 640, 65536, False),
    (1, 0.01, 700, 480, 640, 1413600, True),
    (1, 0.01, 2048, 480, 640, 3840000, True),
    (1, 0.01, 2049, 480, 640, 65536, False),
    (1, 2.3, 1073741824, 480, 640, 65540, False),
    (1, 2.3, 700, 480, 640, 1413600, True),
    (1, 2.3, 2048, 480, 640, 3840000, True),
    (1, 2.3, 2049, 480, 640, 65540, False),
    (1000, None, 1073741824, 480, 640, 113536, False),
    (1000, None, 700, 480, 640, 1413600, True),
    (1000, None, 2048, 480, 640, 3840000, True),
    (1000, None, 2049, 480, 640, 113536, False),
    (1000, 0.01, 1073741824, 480, 640, 65556, False),
    (1000, 0.01, 700, 480, 640, 1413600, True),
    (1000, 0.01, 2048, 480, 640, 3840000, True),
    (1000, 0.01, 2049, 480, 640, 65556, False),
    (1000, 2.3, 1073741824, 480, 640, 70136, False),
    (1000, 2.3, 700, 480, 640, 1413600, True),
    (1000, 2.3, 2048, 480, 640, 3840000, True),
    (1000, 2.3, 2049, 480, 640, 70136, False),
    (157613, None, 1073741824, 480, 640, 7630960, False),
    (157613, None, 700, 480, 640, 7630960, True),
    (157613, None, 2048, 480, 640, 7630960, True),
    (157613, None, 2049, 480, 640, 7630960, False),
    (157613, 0.01, 1073741824, 480, 640, 68688, False),
    (157613, 0.01, 700, 480, 640, 1413600, True),
    (157613, 0.01, 2048, 480, 640, 3840000, True),
    (157613, 0.01, 2049, 480, 640, 68688, False),
    (157613, 2.3, 1073741824, 480, 640, 790555, False),
    (157613, 2.3, 700, 480, 640, 1413600, True),
    (157613, 2.3, 2048, 480, 640, 3840000, True),
    (157613, 2.3, 2049, 480, 640, 790555, False),
    (1000000, None, 1073741824, 480, 640, 48065536, False),
    (1000000, None, 700, 480, 640, 48065536, True),
    (1000000, None, 2048, 480, 640, 48065536, True),
    (1000000, None, 2049, 480, 640, 48065536, False),
    (1000000, 0.01, 1073741824, 480, 640, 85536, False),
    (1000000, 0.01, 700, 480, 640, 1413600, True),
    (1000000, 0.01, 2048, 480, 640, 3840000, True),
    (1000000, 0.01, 2049, 480, 640, 85536, False),
    (1000000, 2.3, 1073741824, 480, 640, 4665536, False),
    (1000000, 2.3, 700, 480, 640, 4665536, True),
    (1000000, 2.3, 2048, 480, 640, 4665536, True),
    (1000000, 2.3, 2049, 480, 640, 4665536, False),
    (255, None, 1, 48, 64, 77776, True),
    (255, None, 2048, 48, 64, 77776, True),
    (255, 0.01, 1, 48, 64, 65541, True),
    (255, 0.01, 2048, 48, 64, 65541, True),
    (257, None, 1, 48, 64, 77872, True),
    (257, None, 2048, 48, 64, 77872, True),
    (257, 0.01, 1, 48, 64, 65541, True),
    (257, 0.01, 2048, 48, 64, 65541, True),
    (1000000, None, 1, 48, 64, 48065536, True),
    (1000000, None, 2048, 48, 64, 48065536, True),
    (1000000, 0.01, 1, 48, 64, 250049, True),
    (1000000, 0.01, 2048, 48, 64, 250049, True),
    (524289, 0.01, 700, 1080, 1920, 9612480, True),
    (1048577, 0.01, 700, 1080, 1920, 9612480, True),
    (4194304, 0.01, 700, 1080, 1920, 149422, False),
    (4194305, 0.01, 700, 1080, 1920, 149422, False),
    (1048577, 0.01, 2048, 480, 640, 86507, False),
)


def test_engine_sizing_picks_the_capacities_it_always_picked():
    assert len({(s[5], s[6]) for s in SIZING}) > 20
    for P, ratio, mtl, H, W, want, direct in SIZING:
        assert FusedEngine.sizing(P, ratio, mtl, H, W) == (want, direct), (P, ratio, mtl, H, W)
    floor = [s for s in SIZING if s[6] and s[5] == ((s[0] + 255) // 256) * 64 + 1]
    assert floor and all(s[0] == 1000000 and s[1] == 0.01 for s in floor)
    assert any(s[6] for s in SIZING if s[2] == 2048) and not any(s[6] for s in SIZING if s[2] == 2049)
