"""Host reference of the per-tile sort and the sixteen 4x4-block lists (csrc/sort_tile.h sort_tile_body), read back from the
kernels' state buffers and checked exactly.

Keys are unique (depth bits, id), so any correct sort yields exactly one order, and every list the emitters write has one correct
answer.  For a tile this module computes that answer on the host and compares it with what the kernels left behind:
  * the sorted bin words (block mask | per-tile record << 32): the records are unique per (Gaussian, tile) pair, so their sequence
    pins the depth order itself;
  * the block masks, against a float32 mirror of tile_mask.h (mask_consts, block_rect, tile_block_mask_in_rect) evaluated at
    both ends of the error band of the hardware log (see TAU_ULPS);
  * the sixteen id lists and subcount;
  * an independent float64 property: no block that a pair's mask leaves out holds a pixel where that splat reaches alpha 1/255.

The buffer readers mirror csrc/mm3dgs_common.h (geom_view, image_view, bin_view); keep them in step with it.
Every array this module reads is sliced on the device first: at 1080p the block lists alone hold over a gigabyte."""
import numpy as np
import torch

TILE = 16
NLIST = 16
SPLAT_F = 12
ALPHA_MIN = 1.0 / 255.0
DIRECT_DROP_OWN = 4          # fused.hip slam_bin_pairs: a splat's first four pairs may be dropped when their mask is empty ...
DIRECT_DROP_MAX_AREA = 32    # ... if its rectangle covers 32 tiles or fewer (the wave-cooperative path lists every pair)
PREPROCESS_GROUP = 256       # Gaussians per projection workgroup (block_tiles / trec_cap granularity)
# __logf on gfx950 is v_log_f32 (the hardware log2, specified to 1 ulp) followed by a product with ln 2 carried in two parts (v_mul /
# v_fma / v_fmamk / v_fmac: the product is formed in extended precision and rounded once, <= 0.5 ulp).  The device tau therefore lies
# within 1.5 ulp of the float64 log rounded to float32 (itself 0.5 ulp from the exact value); 2 ulp on either side bounds it.
TAU_ULPS = 2
# Relative margin below 1/255 that the float64 property check demands of every block left out of a mask.  The mask bounds carry a
# 1.0002 (box) / 1.0004 (disc) factor on the radius (tile_mask.h), so a left-out block sits at least ~4e-4 tau below the threshold in
# the exponent; 1e-7 only absorbs the float64 evaluation itself.
PROPERTY_MARGIN = 1e-7


def _al(v, a=256):
    return (int(v) + a - 1) // a * a


# ---- buffer layouts (csrc/mm3dgs_common.h) -------------------------------------------------------------------------------
def geom_offsets(P):
    """Byte offsets of geom_view's arrays for a buffer sized for P Gaussians."""
    P = max(int(P), 1)
    nb = (P + 255) // 256 + 1
    o, c = {}, 0
    for name, size in (("splat", P * SPLAT_F * 4), ("depth", P * 4), ("rect", P * 8), ("clamped", P), ("tileoff", P * 4),
                       ("block_tiles", nb * 4), ("poserec", 0)):
        o[name] = c
        c += _al(size)
    return o


def image_offsets(H, W):
    T = ((W + TILE - 1) // TILE) * ((H + TILE - 1) // TILE)
    o, c = {}, 0
    for name, size in (("hdr", 256), ("tile_count", T * 4), ("ranges", (T + 1) * 4), ("cursor", T * 4), ("subcount", T * NLIST * 4),
                       ("final_T", H * W * 4), ("n_contrib", H * W * 4), ("tile_order", 0)):
        o[name] = c
        c += _al(size) if name != "hdr" else 256
    return o


def bin_offsets(N):
    N = max(int(N), 1)
    o, c = {}, 0
    for name, size in (("keys", N * 8), ("sublist", N * NLIST * 8), ("submask", N * 2), ("payload", N * 8), ("trec", 0)):
        o[name] = c
        c += _al(size)
    return o


HDR = ("num_rendered", "overflow", "max_tile_len", "max_num_rendered", "fwd_wave_iters", "bwd_wave_iters", "bwd_wave_visits",
       "bin_cap", "reserved8", "tile_order_tiles", "overflow_seen", "mean_wave_steps")


def _u32(buf, off, n):
    return buf[off:off + 4 * n].view(torch.int32)


class ListState:
    """The kernels' state after one render, read through device slices.  geom / img / binning: the uint8 state tensors; P: the
    Gaussian count of the render; N: the binning capacity; radii: [P] int32."""

    def __init__(self, geom, img, binning, P, H, W, N, radii):
        self.P, self.H, self.W, self.N = int(P), int(H), int(W), int(N)
        self.gx, self.gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
        self.T = self.gx * self.gy
        self.geom, self.img, self.binning = geom, img, binning
        go, io = geom_offsets(P), image_offsets(H, W)      # (the kernels lay geom_state out for the render's P, whatever it was sized for)
        self.bo = bin_offsets(N)
        P = self.P
        h = img[:48].view(torch.int32).cpu().numpy().astype(np.int64) & 0xffffffff
        self.hdr = {k: int(h[i]) for i, k in enumerate(HDR)}
        T = self.T
        self.tile_count = _u32(img, io["tile_count"], T).cpu().numpy().astype(np.int64)
        self.ranges = (_u32(img, io["ranges"], T + 1).cpu().numpy().astype(np.int64) & 0xffffffff)
        self.cursor = _u32(img, io["cursor"], T).cpu().numpy().astype(np.int64)
        self.subcount = _u32(img, io["subcount"], T * NLIST).cpu().numpy().astype(np.int64).reshape(T, NLIST)
        # per-Gaussian arrays stay on the device (at 3 M Gaussians the splat records are 144 MB); the readers gather what a tile needs
        self.splat = geom[go["splat"]:go["splat"] + P * SPLAT_F * 4].view(torch.float32).view(P, SPLAT_F)
        self.depth = geom[go["depth"]:go["depth"] + 4 * P].view(torch.float32)
        rect = geom[go["rect"]:go["rect"] + 8 * P].view(torch.int32).view(P, 2).long() & 0xffffffff
        self.rect = torch.stack([rect[:, 0] & 0xffff, rect[:, 0] >> 16, rect[:, 1] & 0xffff, rect[:, 1] >> 16], 1)   # minx miny maxx maxy
        self.tileoff = _u32(geom, go["tileoff"], P).long()
        self.block_tiles = _u32(geom, go["block_tiles"], (P + 255) // 256 + 1).long()
        self.clamped = geom[go["clamped"]:go["clamped"] + P]
        self.radii = radii[:P]

    # ---- tile_span semantics (mm3dgs_common.h) --------------------------------------------------------------------------
    def span(self, tile):
        cap = self.hdr["bin_cap"]
        a, b = int(self.ranges[tile]), int(self.ranges[tile + 1])
        if cap:
            return tile * cap, min(a, cap)
        start = min(a, self.N)
        return start, min(b, self.N) - start

    def area(self):
        r = self.rect
        w, h = r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
        return torch.where((w > 0) & (h > 0), w * h, torch.zeros_like(w))

    def read_tiles(self, tiles):
        """Per tile: start, len, the sorted bin words [len] (uint64) and the sixteen id lists (the .y words asserted zero).  One
        gather on the device for all tiles."""
        keys64 = self.binning[self.bo["keys"]:self.bo["keys"] + 8 * self.N].view(torch.int64)
        sub32 = self.binning[self.bo["sublist"]:self.bo["sublist"] + 8 * NLIST * self.N].view(torch.int32)
        kidx, sidx, spans = [], [], []
        for t in tiles:
            start, ln = self.span(int(t))
            spans.append((start, ln))
            kidx.append(np.arange(start, start + ln, dtype=np.int64))
            for L in range(NLIST):
                n = int(self.subcount[t, L])
                assert 0 <= n <= ln, (t, L, n, ln)
                base = NLIST * start + L * ln
                sidx.append(np.arange(2 * base, 2 * (base + n), dtype=np.int64))
        kidx = np.concatenate(kidx) if kidx else np.zeros(0, np.int64)
        sidx = np.concatenate(sidx) if sidx else np.zeros(0, np.int64)
        dev = keys64.device
        kv = keys64[torch.from_numpy(kidx).to(dev)].cpu().numpy().view(np.uint64)
        sv = sub32[torch.from_numpy(sidx).to(dev)].cpu().numpy().reshape(-1, 2)
        assert not sv[:, 1].any(), "block list entries must have a zero .y word"
        out, ka, sa = {}, 0, 0
        for t, (start, ln) in zip(tiles, spans):
            lists = []
            for L in range(NLIST):
                n = int(self.subcount[t, L])
                lists.append(sv[sa:sa + n, 0].astype(np.int64))
                sa += n
            out[int(t)] = dict(start=start, len=ln, words=kv[ka:ka + ln], lists=lists)
            ka += ln
        return out

    def candidates(self, tiles):
        """Per tile: ids (int64, ascending) of the Gaussians with radii > 0 whose tile rectangle holds the tile, and their pair
        index k inside the rectangle (row-major)."""
        r = self.rect
        vis = self.radii > 0
        out = {}
        for t in tiles:
            tx, ty = int(t) % self.gx, int(t) // self.gx
            m = vis & (r[:, 0] <= tx) & (tx < r[:, 2]) & (r[:, 1] <= ty) & (ty < r[:, 3])
            ids = torch.nonzero(m).flatten()
            rr = r[ids]
            k = (ty - rr[:, 1]) * (rr[:, 2] - rr[:, 0]) + (tx - rr[:, 0])
            out[int(t)] = (ids.cpu().numpy(), k.cpu().numpy())
        return out


# ---- float32 mirror of tile_mask.h / block_rect ---------------------------------------------------------------------------
f32 = np.float32


def tau_band(opacity, ulps=TAU_ULPS):
    """(tau_lo, tau_hi): the float32 log(255 o) (255 o rounded like __fmul_rn) shifted by -ulps / +ulps ulp -- the band the device's
    __logf lies in.  log(1) is 0 exactly on both sides."""
    x = (f32(255.0) * opacity.astype(f32)).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.log(x.astype(np.float64)).astype(f32)
    lo, hi = t.copy(), t.copy()
    for _ in range(ulps):
        lo = np.nextafter(lo, f32(-np.inf))
        hi = np.nextafter(hi, f32(np.inf))
    exact = x == f32(1.0)
    lo[exact] = 0.0
    hi[exact] = 0.0
    return lo, hi


def _ceil_i(v):
    return np.clip(np.ceil(v.astype(np.float64)), -2 ** 31, 2 ** 31 - 1).astype(np.int64)


def _floor_i(v):
    return np.clip(np.floor(v.astype(np.float64)), -2 ** 31, 2 ** 31 - 1).astype(np.int64)


def block_rect(A, B, rect, tau):
    """mm3dgs_common.h block_rect, vectorised: (bx0, by0, bw, bh) int64 arrays."""
    X0, Y0, X1, Y1 = rect[:, 0] * 4, rect[:, 1] * 4, rect[:, 2] * 4, rect[:, 3] * 4
    bx0, by0, bw, bh = X0.copy(), Y0.copy(), X1 - X0, Y1 - Y0
    empty = (bw <= 0) | (bh <= 0)
    with np.errstate(all="ignore"):
        det = (A[:, 2] * B[:, 0]).astype(f32) - (A[:, 3] * A[:, 3]).astype(f32)
        degenerate = ~(det > 0)
        dead = ~degenerate & ~(tau > 0)
        k = ((f32(2.0) * tau).astype(f32) / det).astype(f32)
        hx = (np.sqrt((k * B[:, 0]).astype(f32)) * f32(1.0002)).astype(f32) + f32(0.012)
        hy = (np.sqrt((k * A[:, 2]).astype(f32)) * f32(1.0002)).astype(f32) + f32(0.012)
        cbx0 = np.maximum(X0, _ceil_i((((A[:, 0] - hx).astype(f32) - f32(3.0)).astype(f32) * f32(0.25)).astype(f32)))
        cbx1 = np.minimum(X1 - 1, _floor_i(((A[:, 0] + hx).astype(f32) * f32(0.25)).astype(f32)))
        cby0 = np.maximum(Y0, _ceil_i((((A[:, 1] - hy).astype(f32) - f32(3.0)).astype(f32) * f32(0.25)).astype(f32)))
        cby1 = np.minimum(Y1 - 1, _floor_i(((A[:, 1] + hy).astype(f32) * f32(0.25)).astype(f32)))
    live = ~empty & ~degenerate & ~dead
    cbw, cbh = np.maximum(cbx1 - cbx0 + 1, 0), np.maximum(cby1 - cby0 + 1, 0)
    zero = (cbw == 0) | (cbh == 0)
    bx0 = np.where(live, cbx0, bx0)
    by0 = np.where(live, cby0, by0)
    bw = np.where(empty | dead, 0, np.where(live, np.where(zero, 0, cbw), bw))
    bh = np.where(empty | dead, 0, np.where(live, np.where(zero, 0, cbh), bh))
    return bx0, by0, bw, bh


def mask_consts(A, B, tau):
    """tile_mask.h mask_consts, vectorised: (cx, cy, hx, hy, r2, mode)."""
    with np.errstate(all="ignore"):
        det = (A[:, 2] * B[:, 0]).astype(f32) - (A[:, 3] * A[:, 3]).astype(f32)
        mode = np.where(~(det > 0), 2, np.where(~(tau > 0), 0, 1))
        t2 = (f32(2.0) * tau).astype(f32)
        k = (t2 / det).astype(f32)
        hx = (np.sqrt((k * B[:, 0]).astype(f32)) * f32(1.0002)).astype(f32) + f32(0.002)
        hy = (np.sqrt((k * A[:, 2]).astype(f32)) * f32(1.0002)).astype(f32) + f32(0.002)
        sxx, syy = (B[:, 0] / det).astype(f32), (A[:, 2] / det).astype(f32)
        mid = (f32(0.5) * (sxx + syy).astype(f32)).astype(f32)
        disc = np.maximum(((mid * mid).astype(f32) - (f32(1.0) / det).astype(f32)).astype(f32), f32(0.0))
        lam = (mid + np.sqrt(disc)).astype(f32)
        r2 = (((t2 * lam).astype(f32) * f32(1.0004)).astype(f32) + f32(0.01)).astype(f32)
    return A[:, 0].astype(f32), A[:, 1].astype(f32), hx.astype(f32), hy.astype(f32), r2, mode


def _bit(kx, my):
    return 4 * ((my >> 1) * 2 + (kx >> 1)) + (my & 1) * 2 + (kx & 1)


_YY, _XX = np.meshgrid(np.arange(TILE), np.arange(TILE), indexing="ij")
PIXEL_BIT = np.vectorize(_bit)(_XX // 4, _YY // 4)      # [16,16]: the mask bit of the block that holds tile pixel (y, x)


def tile_block_mask_in_rect(mc, ttx, tty, br):
    """tile_mask.h tile_block_mask_in_rect, vectorised over pairs (ttx, tty int64 arrays): uint32 masks."""
    cx0, cy0, hx, hy, r2, mode = mc
    bx0, by0, bw, bh = br
    with np.errstate(all="ignore"):
        cx = (cx0 - (ttx * TILE).astype(f32)).astype(f32)
        cy = (cy0 - (tty * TILE).astype(f32)).astype(f32)
        bx, by, ex, ey = [], [], [], []
        for q in range(4):
            lo, hi = f32(4.0 * q), f32(4.0 * q + 3.0)
            inx = ((ttx * 4 + q - bx0) >= 0) & ((ttx * 4 + q - bx0) < bw)
            iny = ((tty * 4 + q - by0) >= 0) & ((tty * 4 + q - by0) < bh)
            tx_ = ((cx - hx).astype(f32) <= hi) & ((cx + hx).astype(f32) >= lo)
            ty_ = ((cy - hy).astype(f32) <= hi) & ((cy + hy).astype(f32) >= lo)
            dxq = np.maximum(np.maximum((lo - cx).astype(f32), (cx - hi).astype(f32)), f32(0.0))
            dyq = np.maximum(np.maximum((lo - cy).astype(f32), (cy - hi).astype(f32)), f32(0.0))
            m1 = mode == 1
            bx.append(inx & (~m1 | tx_))
            by.append(iny & (~m1 | ty_))
            ex.append(np.where(m1, (dxq * dxq).astype(f32), f32(0.0)))
            ey.append(np.where(m1, (dyq * dyq).astype(f32), f32(0.0)))
        mask = np.zeros(cx.shape, np.uint32)
        for my in range(4):
            for kx in range(4):
                on = bx[kx] & by[my] & ((mode == 2) | ((ex[kx] + ey[my]).astype(f32) <= r2))
                mask |= np.where(on, np.uint32(1 << _bit(kx, my)), np.uint32(0))
    return np.where(mode == 0, np.uint32(0), mask).astype(np.uint32)


def mask_band(A, B, rect, ttx, tty):
    """(lower, upper) block masks of pairs (A, B [n,4] float32 splat record words, rect [n,4] tile rectangle of the splat, the
    pair's tile): the mirror at tau - TAU_ULPS ulp and at tau + TAU_ULPS ulp.  Every extent grows with tau, so lower is a subset of
    upper; a correct kernel's mask lies between them, and bits set in upper only are the ambiguous ones."""
    lo_t, hi_t = tau_band(B[:, 1])
    out = []
    for tau in (lo_t, hi_t):
        out.append(tile_block_mask_in_rect(mask_consts(A, B, tau), ttx, tty, block_rect(A, B, rect, tau)))
    return out[0], out[1]


def popcount(x):
    x = np.ascontiguousarray(np.asarray(x, np.uint64).ravel()).astype("<u8")
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(1).astype(np.int64)


# ---- float64 property check (no mirror involved) -----------------------------------------------------------------------
def max_alpha_outside(A, B, ttx, tty, masks, chunk=2048):
    """Per pair: the largest float64 alpha (o exp(power), power <= 0, as the compositors evaluate it) over the pixel centres of the
    tile's blocks that `masks` leaves out; 0 where every block is listed.  From the kernel's own float32 splat record."""
    n = A.shape[0]
    if n > chunk:
        return np.concatenate([max_alpha_outside(A[a:a + chunk], B[a:a + chunk], ttx[a:a + chunk], tty[a:a + chunk], masks[a:a + chunk])
                               for a in range(0, n, chunk)])
    if n == 0:
        return np.zeros(0)
    lx = np.arange(TILE, dtype=np.float64)
    px = (ttx[:, None] * TILE).astype(np.float64) + lx[None, :]          # [n,16] pixel columns
    py = (tty[:, None] * TILE).astype(np.float64) + lx[None, :]
    dx = A[:, 0:1].astype(np.float64) - px                                 # [n,16]
    dy = A[:, 1:2].astype(np.float64) - py
    ca, cb, cc, o = (A[:, 2].astype(np.float64), A[:, 3].astype(np.float64), B[:, 0].astype(np.float64), B[:, 1].astype(np.float64))
    power = -0.5 * (ca[:, None, None] * dx[:, None, :] ** 2 + cc[:, None, None] * dy[:, :, None] ** 2) \
        - cb[:, None, None] * dx[:, None, :] * dy[:, :, None]                # [n, y, x]
    alpha = np.where(power <= 0, o[:, None, None] * np.exp(np.minimum(power, 0.0)), 0.0)
    # block of pixel (y, x) -> its bit
    left_out = ((masks.astype(np.int64)[:, None, None] >> PIXEL_BIT[None]) & 1) == 0
    return np.where(left_out, alpha, 0.0).reshape(n, -1).max(1)


# ---- the expected lists of a tile and the comparison ---------------------------------------------------------------------
class Stats:
    def __init__(self):
        self.pairs = 0
        self.tiles = 0
        self.ambiguous_bits = 0
        self.ambiguous_drops = 0
        self.worst_alpha = 0.0
        self.lens = []

    def __repr__(self):
        return (f"tiles={self.tiles} pairs={self.pairs} ambiguous_bits={self.ambiguous_bits} "
                f"({self.ambiguous_bits / max(16 * self.pairs, 1):.1e} of bits) ambiguous_drops={self.ambiguous_drops} "
                f"max_alpha_outside*255={self.worst_alpha * 255:.6f}")


def check_tiles(st: ListState, tiles, direct, trec_cap=0, stats=None):
    """Asserts, for every tile of `tiles`, that the kernels' bin (order via the per-tile records, masks within the mirror's band),
    block lists and subcount are the host reference's, and that every left-out block is below 1/255 in float64.  direct: the
    direct-bin layout (empty-mask drop rule, records per projection workgroup of trec_cap).  Returns `stats` (Stats)."""
    stats = stats if stats is not None else Stats()
    tiles = [int(t) for t in tiles]
    got = st.read_tiles(tiles)
    cand = st.candidates(tiles)
    area = st.area()
    if direct:
        grp = torch.arange(st.P, device=area.device) // PREPROCESS_GROUP
        incl = torch.cumsum(area, 0)
        first = torch.arange(0, st.P, PREPROCESS_GROUP, device=area.device)
        gbase = torch.where(first > 0, incl[(first - 1).clamp(min=0)], torch.zeros_like(first))
        plocal = incl - area - gbase[grp]
        rec_base = torch.where(plocal + area <= trec_cap, grp * trec_cap + plocal, torch.full_like(plocal, -1))
        # the device's own per-Gaussian prefix (tileoff = plocal on this path)
        live = area > 0
        assert torch.equal(st.tileoff[live], plocal[live]), "tileoff differs from the workgroup-local prefix of the rectangle areas"
    else:
        excl = torch.cumsum(area, 0) - area
        rec_base = excl
        live = area > 0
        dev_pidx = st.block_tiles[torch.arange(st.P, device=area.device) // 256] + st.tileoff
        assert torch.equal(dev_pidx[live], excl[live]), "block_tiles + tileoff differ from the Gaussian-major prefix of the rectangle areas"
    all_ids = np.unique(np.concatenate([c[0] for c in cand.values()])) if cand else np.zeros(0, np.int64)
    idx_t = torch.from_numpy(all_ids).to(st.splat.device)
    rec_g = st.splat[idx_t].cpu().numpy()
    dep_g = st.depth[idx_t].cpu().numpy()
    rect_g = st.rect[idx_t].cpu().numpy()
    area_g = area[idx_t].cpu().numpy()
    base_g = rec_base[idx_t].cpu().numpy()
    pos = {int(i): j for j, i in enumerate(all_ids)}
    for t in tiles:
        ids, k = cand[t]
        g = got[t]
        j = np.array([pos[int(i)] for i in ids], np.int64) if ids.size else np.zeros(0, np.int64)
        dbits = dep_g[j].view(np.uint32).astype(np.uint64) if ids.size else np.zeros(0, np.uint64)
        key = (dbits << np.uint64(32)) | ids.astype(np.uint64)
        order = np.argsort(key, kind="stable")
        ids, k, j = ids[order], k[order], j[order]
        A, B = rec_g[j, 0:4].astype(f32), rec_g[j, 4:8].astype(f32)
        ttx = np.full(ids.shape, t % st.gx, np.int64)
        tty = np.full(ids.shape, t // st.gx, np.int64)
        lower, upper = mask_band(A, B, rect_g[j], ttx, tty)
        base = base_g[j]
        if direct:
            recs = np.where(base >= 0, base + k, 0xffffffff).astype(np.int64)
        else:
            recs = np.where(base + k < st.N, base + k, 0xffffffff).astype(np.int64)
        words = g["words"]
        krec = (words >> np.uint64(32)).astype(np.int64)
        kmask = (words & np.uint64(0xffffffff)).astype(np.int64)
        if direct:
            a = area_g[j]
            droppable = (a >= 1) & (a <= DIRECT_DROP_MAX_AREA) & (k < DIRECT_DROP_OWN)
            drop_sure = droppable & (upper == 0)
            maybe = droppable & (lower == 0) & (upper != 0)
            keep = ~drop_sure
            if maybe.any():      # the kernel's __logf decided: the pair is there iff its record is
                stats.ambiguous_drops += int(maybe.sum())
                present = np.isin(recs, krec)
                keep &= ~maybe | present
            ids, k, recs, lower, upper, A, B, ttx, tty = (x[keep] for x in (ids, k, recs, lower, upper, A, B, ttx, tty))
        assert g["len"] == ids.size, f"tile {t}: bin length {g['len']} != {ids.size} expected"
        bad = np.nonzero(krec != recs)[0]
        assert bad.size == 0, f"tile {t} (len {ids.size}): {bad.size} sorted entries carry the wrong record, first at {bad[:8]} " \
                              f"(got {krec[bad[:8]]}, expected {recs[bad[:8]]})"
        lo_ok = (kmask & lower) == lower
        hi_ok = (kmask & ~upper.astype(np.int64)) == 0
        bad = np.nonzero(~(lo_ok & hi_ok))[0]
        assert bad.size == 0, f"tile {t}: {bad.size} block masks outside the float32 mirror's band, first ids {ids[bad[:8]]} " \
                              f"(got {kmask[bad[:8]]}, band {lower[bad[:8]]}..{upper[bad[:8]]})"
        stats.ambiguous_bits += int(popcount((upper & ~lower).astype(np.uint64)).sum())
        for L in range(NLIST):
            exp_ids = ids[((kmask >> L) & 1) == 1]
            lst = g["lists"][L]
            assert st.subcount[t, L] == exp_ids.size, f"tile {t} list {L}: subcount {st.subcount[t, L]} != {exp_ids.size}"
            assert np.array_equal(lst, exp_ids), f"tile {t} list {L}: ids differ at {np.nonzero(lst != exp_ids)[0][:8]}"
        amax = max_alpha_outside(A, B, ttx, tty, kmask.astype(np.uint32))
        if amax.size:
            w = int(np.argmax(amax))
            stats.worst_alpha = max(stats.worst_alpha, float(amax[w]))
            assert amax[w] < ALPHA_MIN * (1.0 - PROPERTY_MARGIN), \
                f"tile {t}: splat {ids[w]} reaches alpha {amax[w]:.9g} (1/255 = {ALPHA_MIN:.9g}) in a block its mask leaves out"
        stats.pairs += int(ids.size)
        stats.tiles += 1
        stats.lens.append(int(ids.size))
    return stats


def tier_counts(lens, edges=(1024, 2048, 16384)):
    """Tiles per sort tier: len <= 1024 (rank sort), (1024, 2048], (2048, 16384], > 16384 (0-length tiles excluded)."""
    lens = np.asarray(lens)
    lens = lens[lens > 0]
    out, lo = [], 0
    for e in edges:
        out.append(int(((lens > lo) & (lens <= e)).sum()))
        lo = e
    out.append(int((lens > lo).sum()))
    return out


# ---- host-only helpers (reference self-checks) ---------------------------------------------------------------------------
def expected_order(depth, rect, radii, tile, gx):
    """Ids of the Gaussians with radii > 0 whose rectangle holds `tile`, in (float32 depth bits, id) order."""
    tx, ty = tile % gx, tile // gx
    m = (radii > 0) & (rect[:, 0] <= tx) & (tx < rect[:, 2]) & (rect[:, 1] <= ty) & (ty < rect[:, 3])
    ids = np.nonzero(m)[0]
    key = (depth[ids].astype(f32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
    return ids[np.argsort(key, kind="stable")]
