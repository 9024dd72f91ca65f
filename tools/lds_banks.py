#!/usr/bin/env python3
"""LDS bank-conflict model for ds_read_b128 on gfx950 (lane groups per MI355X_MICROARCH.md §LDS):
LDS cycles per wave-instruction (4 = conflict-free) of the conv2 core operand reads under the
plain swz128 key and the padded-image swzpad key (csrc/kernels/common.h)."""

G128 = [list(range(0,4))+list(range(12,16))+list(range(20,28)),
        list(range(4,12))+list(range(16,20))+list(range(28,32)),
        list(range(32,36))+list(range(44,48))+list(range(52,60)),
        list(range(36,44))+list(range(48,52))+list(range(60,64))]
def cycles(addr):  # addr: byte address per lane (64)
    tot = 0
    for grp in G128:
        banks = {}
        for l in grp:
            for d in range(4):
                dw = addr[l] // 4 + d
                banks.setdefault(dw % 64, set()).add(dw)
        tot += max(len(v) for v in banks.values())
    return tot  # 4 = conflict-free
def swz_old(pix, c): return pix * 64 + ((c ^ (pix & 7)) << 3)
def swz_new(pix, c): return pix * 64 + ((c ^ ((pix + 4 * (pix >> 4)) & 7)) << 3)
def conv2_B(swz):
    res = []
    for NPX, pg in ((3, 0), (2, 1), (2, 2), (2, 3)):
        for t in range(NPX):
            for kh in range(5):
                for kw in range(5):
                    for s in range(2):
                        addr = []
                        for lane in range(64):
                            g, li = lane >> 4, lane & 15
                            px = 16 * (pg + 4 * t) + li
                            px = min(px, 143)
                            y = px // 12; pb = y * 16 + (px - y * 12)
                            addr.append(2 * swz(pb + kh * 16 + kw, 4 * s + g))
                        res.append(cycles(addr))
    return sum(res) / len(res)
def conv2_A():
    res = []
    for cp in range(2):
        for kw in range(5):
            for s in range(2):
                for h in range(2):
                    addr = []
                    for lane in range(64):
                        g, li = lane >> 4, lane & 15
                        row = 32 * cp + 16 * h + li
                        c = ((kw * 8 + s * 4 + g) ^ (li & 7)) * 8
                        addr.append(2 * (row * 320 + c))
                    res.append(cycles(addr))
    return sum(res) / len(res)
print("B old", conv2_B(swz_old), "B new", conv2_B(swz_new), "A", conv2_A())

# --- grouped GEMM (cnn_gemm.hip) and head (cnn_head.hip) operand images ---------------------------
G64 = [list(range(0, 32)), list(range(32, 64))]      # ds_read_b64 / ds_read_b64_tr_b16 lane groups


def cycles_g(addr, groups, ndw):
    tot = 0
    for grp in groups:
        banks = {}
        for l in grp:
            for d in range(ndw):
                dw = addr[l] // 4 + d
                banks.setdefault(dw % 64, set()).add(dw)
        tot += max(len(v) for v in banks.values())
    return tot


def gemm_kmajor(ld):            # lds_b128(sm + (rr0 + li) * KC_LD + kk * 32 + 8 g): ideal 4
    r = [cycles_g([2 * ((rr0 + (l & 15)) * ld + kk * 32 + 8 * (l >> 4)) for l in range(64)], G128, 4)
         for kk in range(4) for rr0 in (0, 16, 32, 48)]
    return sum(r) / len(r)


def mswz(row, col, ld=64):      # cnn_gemm.hip mswz
    f = 2 * (((row >> 1) & 1) | (((row >> 3) & 1) << 1))
    return row * ld + (((col >> 3) ^ f) << 3) + (col & 7)


def gemm_mmajor(off):           # tr_frag rows kk*32 + 8g + hh + q, cols rr0 + 4p: ideal 2
    r = []
    for kk in range(4):
        for rr0 in (0, 16, 32, 48):
            for hh in (0, 4):
                r.append(cycles_g([2 * off(kk * 32 + 8 * (l >> 4) + hh + ((l & 15) >> 2), rr0 + 4 * (l & 3))
                                   for l in range(64)], G64, 2))
    return sum(r) / len(r)


def w2swz(row, col, ld=384):    # cnn_head.hip w2swz
    return row * ld + (((col >> 3) ^ (2 * (row & 3) + 8 * ((row >> 3) & 1))) << 3) + (col & 7)


def head_reads(off):            # (b) b128 row fragments, ideal 4; (f) tr column fragments, ideal 2
    rb = [cycles_g([2 * off(16 * w + (l & 15), 8 * (l >> 4) + 32 * ks) for l in range(64)], G128, 4)
          for w in range(12) for ks in range(12)]
    rt = [cycles_g([2 * off(32 * ks + 8 * (l >> 4) + hh + ((l & 15) >> 2), 16 * w + 4 * (l & 3)) for l in range(64)],
                   G64, 2) for w in range(24) for ks in range(6) for hh in (0, 4)]
    return sum(rb) / len(rb), sum(rt) / len(rt)


print("gemm k-major b128: KC_LD 136 ->", gemm_kmajor(136), " KC_LD 144 ->", gemm_kmajor(144))
print("gemm m-major tr: MC_LD 72 ->", gemm_mmajor(lambda r, c: r * 72 + c), " swizzled 64 ->", gemm_mmajor(mswz))
print("head fc2 (b128, tr): W2_LD 392 ->", head_reads(lambda r, c: r * 392 + c), " swizzled 384 ->", head_reads(w2swz))


# --- max-pool reads of a conv output image (conv_common.h pool_emit) ------------------------------
# r5: the conflict-free variant modelled here (rows px, px ^ 1 swapped for bit 1 of px + two pixels x 8
# chunks per lane group) measured SLOWER on the GPU (pool1 2.44 -> 2.88 us, step +0.5 us,
# profiles/r5_pool_swz_ab.txt): the pool is VALU-bound and the permuted lanes cost the stores their
# contiguity, so the shipped pool keeps lane -> (lane >> 3, lane & 7) and swz128.
def _pool_swz(p, c, swap):
    q = p ^ ((p >> 1) & 1) if swap else p
    return q * 64 + ((c ^ (q & 7)) << 3)


_GI = {l: (G, i) for G, grp in enumerate(G128) for i, l in enumerate(grp)}


def pool_reads(H, swap, grouped):
    """LDS cycles per ds_read_b128 of the 9 tap reads; grouped: pool_emit's lane order (two pixels
    x 8 chunks per lane group) instead of lane -> (lane >> 3, lane & 7)."""
    HO, res = H // 2, []
    for wv in range(HO * HO // 8):
        for d in range(9):
            addr = []
            for l in range(64):
                G, i = _GI[l]
                ql, c = (2 * G + (i >> 3), i & 7) if grouped else (l >> 3, l & 7)
                py, px = divmod(8 * wv + ql, HO)
                y, x = min(2 * py + d // 3, H - 1), min(2 * px + d % 3, H - 1)
                addr.append(2 * _pool_swz(y * H + x, c, swap))
            res.append(cycles(addr))
    return sum(res) / len(res)


for H in (24, 12):
    print(f"pool{1 if H == 24 else 2} reads: r4 {pool_reads(H, False, False):.1f}  swzpool + grouped lanes {pool_reads(H, True, True):.1f}")


# --- fp32 conv2 weight gradient (f32_conv.hip k_f32_conv2_wgrad): one 4-byte word per lane ----------------
# lane (q, r) of wave j reads word j of channel chunk r of padded pixel (py, px + q): passes per wave read
# (1 = the 64 lanes hit 64 distinct banks) under the p1_off chunk swizzle of k_f32_conv2 and in the channel
# planes the kernel uses (plane j = [16][16][16] words, word 16 * pixel + r).
def wgrad_reads(off):
    res = []
    for j in range(4):
        for py in range(16):
            for px in range(13):
                banks = {}
                for l in range(64):
                    dw = off(py, px + (l >> 4), l & 15, j)
                    banks.setdefault(dw % 64, set()).add(dw)
                res.append(max(len(v) for v in banks.values()))
    return sum(res) / len(res), max(res)


def p1_word(py, px, c, j): return (py * 16 + px) * 64 + ((c ^ ((px & 3) | ((py & 3) << 2))) << 2) + j
def plane_word(py, px, c, j): return j * 4096 + (py * 16 + px) * 16 + c


print("wgrad 4-byte reads (mean, worst passes): p1_off swizzle ->", wgrad_reads(p1_word), " channel planes ->", wgrad_reads(plane_word))


# --- fp32 conv1 backward (f32_conv1.hip k_f32_conv1_wgrad): one 4-byte word per lane, both operands -----------
# First operand: lane (q, r) of row tile t reads im2col row m = 16 t + r of pixel (y, x0 + q) of the zero-padded
# [28][pitch] image, word (y + kh) * pitch + (x0 + q + kw) * 3 + ci (rows 75 .. 79 read word 0 and are replaced);
# equal words are one broadcast.  Second operand: word 16 * (pixel + q) + r of channel-tile plane nt against the
# pixel-major band [pixel][64].
def conv1_x_reads(pitch):
    res = []
    for t in range(5):
        for y in range(24):
            for x0 in range(0, 24, 4):
                banks = {}
                for l in range(64):
                    q, m = l >> 4, 16 * t + (l & 15)
                    tap, ci = divmod(min(m, 74), 3)
                    dw = (y + tap // 5) * pitch + (x0 + q + tap % 5) * 3 + ci if m < 75 else 0
                    banks.setdefault(dw % 64, set()).add(dw)
                res.append(max(len(v) for v in banks.values()))
    return sum(res) / len(res), max(res)


def conv1_dy_reads(off):
    res = []
    for nt in range(4):
        for pix in range(0, 144, 4):
            banks = {}
            for l in range(64):
                dw = off(pix + (l >> 4), nt, l & 15)
                banks.setdefault(dw % 64, set()).add(dw)
            res.append(max(len(v) for v in banks.values()))
    return sum(res) / len(res), max(res)


print("conv1 wgrad x reads (mean, worst passes): pitch 84 ->", conv1_x_reads(84), " pitch 88 ->", conv1_x_reads(88))
print("conv1 wgrad dy reads (mean, worst passes): [pixel][64] ->", conv1_dy_reads(lambda p, nt, r: p * 64 + 16 * nt + r),
      " channel-tile planes ->", conv1_dy_reads(lambda p, nt, r: nt * 2320 + p * 16 + r))


# --- fp32 fc tail kernels (f32_fc.hip fc_core): ds_read_b128 of A[r][k0 + 4 q .. + 3] from a [16][pitch] fp32 tile ---
def fc_tail_reads(pitch):
    return cycles_g([4 * ((l & 15) * pitch + 4 * (l >> 4)) for l in range(64)], G128, 4)


print("fc tail A-tile b128 reads (cycles, 4 = conflict-free):",
      ", ".join(f"pitch {p} -> {fc_tail_reads(p)}" for p in (384, 388, 196, 400, 404)))
