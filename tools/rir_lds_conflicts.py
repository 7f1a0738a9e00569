#!/usr/bin/env python3
"""Bank-conflict model of the CDNA4 LDS (tools/lds_conflicts.py: `cycles`) applied to the stages of csrc/rir.hip: LDS cycles of a wave's
8-byte reads and writes per stage against the conflict-free count, for each transform size.  A butterfly of span s reads and writes the
complex values g + j + m s (m = 0 .. 3; dword address 2 x index); the pair stage works on positions pk = 4 (u / 2) + (u & 1) and
pm = rev(H - rev(pk)).  usage: python tools/rir_lds_conflicts.py"""
import contextlib
import io
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
with contextlib.redirect_stdout(io.StringIO()):          # the frontend's own report
    from lds_conflicts import cycles


def rev(k, D):
    r = 0
    for _ in range(D):
        r = (r << 2) | (k & 3)
        k >>= 2
    return r


def stage(s, waves=4):
    """(read cycles, write cycles, ideal of either) of `waves` waves' butterflies of span s, summed over the four points"""
    rd = wr = ideal = 0
    for w in range(waves):
        for m in range(4):
            addr = {}
            for lane in range(64):
                u = 64 * w + lane
                j = u & (s - 1)
                addr[lane] = 2 * (((u - j) << 2) + j + m * s)
            r, i = cycles("r64", addr)
            rd += r; ideal += i
            wr += cycles("w64", addr)[0]
    return rd, wr, ideal


def pair(M, waves=8):
    H, D = M // 2, {2048: 5, 8192: 6, 32768: 7}[M]
    out = {"pk": [0, 0, 0], "pm": [0, 0, 0]}
    for w in range(1, waves + 1):                         # wave 0 holds the special task 0
        pk, pm = {}, {}
        for lane in range(64):
            u = 64 * w + lane
            p = ((u >> 1) << 2) | (u & 1)
            pk[lane], pm[lane] = 2 * p, 2 * rev(H - rev(p, D), D)
        for name, addr in (("pk", pk), ("pm", pm)):
            r, i = cycles("r64", addr)
            out[name][0] += r; out[name][1] += cycles("w64", addr)[0]; out[name][2] += i
    return out


def main():
    for M in (2048, 8192, 32768):
        H = M // 2
        print(f"M = {M}")
        s = H // 4
        while s >= 1:
            rd, wr, ideal = stage(s)
            print(f"  span {s:5d}: ds_read_b64 {rd / ideal:.2f} x ideal, ds_write_b64 {wr / (2 * ideal):.2f} x ideal")
            s //= 4
        p = pair(M)
        for name in ("pk", "pm"):
            rd, wr, ideal = p[name]
            print(f"  pair {name}:    ds_read_b64 {rd / ideal:.2f} x ideal, ds_write_b64 {wr / (2 * ideal):.2f} x ideal")


if __name__ == "__main__":
    main()
