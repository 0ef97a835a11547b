"""An integer model of csrc/kernels_sqrt.hpp over the words that tables_sqrt.hpp builds (tests/cpp/host_tables_dump's mode `sqrt`):
sqrt_core, k_sqrt and k_randbit_finalize with the kernel's window order, its negw corrections and its key look-up, every product a
plain modular product of the decoded constants.  `bug` makes a wrong copy of the MODEL (never of the kernel), to show that the sweep
of tests/test_host_tables.py over tests/sqrt_inputs.py notices:
    "no_correction"  window 1 looks up g^(2^16) without window 0's correction
    "wide_mask"      E = (-L/2) masked with 2^32 - 1 instead of 2^31 - 1
    "swapped_rows"   negw rows 0 and 1 exchanged"""
import struct

from tests import randbit_ref as RB

KEY_MUL = 0x9E3779B97F4A7C15       # SQRT_KEY_MUL (csrc/sqrt_args.hpp)
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
IMPLS = {"fr-u29": (RB.P_FR, 9, 29, 261), "fr-sat32": (RB.P_FR, 8, 32, 256), "gl": (RB.P_GL, 2, 32, 0)}   # p, limbs, limb bits, log2 of the radix
LAYOUT = ("negw", "posw", "r2", "one_p", "half", "half_p", "e_sqrt", "e_inv", "keyt", "kbits", "kshift", "bits_sqrt", "bits_inv", "nl", "words")


def parse(raw):
    """the tool's output -> (layout dict, the table's 32-bit words)"""
    head, _, body = raw.partition(b"\n")
    tok = head.split()
    assert tok[0] == b"sqrt" and len(tok) == len(LAYOUT) + 1
    lay = dict(zip(LAYOUT, map(int, tok[1:])))
    assert len(body) == 4 * lay["words"]
    return lay, list(struct.unpack(f"<{lay['words']}I", body))


class Model:
    def __init__(self, impl, lay, words, bug=None):
        self.p, self.nl, self.lb, rbits = IMPLS[impl]
        assert lay["nl"] == self.nl
        p = self.p
        self.R = pow(2, rbits, p)
        self.Rinv = pow(self.R, p - 2, p)
        self.lay, self.words, self.bug = lay, words, bug
        self.negw = [[self.const(lay["negw"] + (256 * m + j) * self.nl) for j in range(256)] for m in range(3)]
        self.posw = [[self.const(lay["posw"] + (256 * m + j) * self.nl) for j in range(256)] for m in range(4)]
        if bug == "swapped_rows":
            self.negw[0], self.negw[1] = self.negw[1], self.negw[0]
        self.half = self.const(lay["half"])
        self.half_p = self.plain(lay["half_p"])
        self.e_sqrt = sum(w << (32 * i) for i, w in enumerate(words[lay["e_sqrt"]:lay["e_sqrt"] + 8]))
        self.e_inv = sum(w << (32 * i) for i, w in enumerate(words[lay["e_inv"]:lay["e_inv"] + 8]))
        kt = words[lay["keyt"]:]
        self.keyt = b"".join(struct.pack("<I", w) for w in kt)
        self.kshift, self.kmask = lay["kshift"], (1 << lay["kbits"]) - 1

    # ---- the constants' forms --------------------------------------------------------------------------------------------------------
    def limbs_value(self, off):
        ws = self.words[off:off + self.nl]
        assert all(w < 1 << self.lb for w in ws)
        return sum(w << (self.lb * i) for i, w in enumerate(ws))

    def plain(self, off):
        v = self.limbs_value(off)
        assert v < self.p
        return v

    def const(self, off):
        """a value stored in the implementation's constant form v Rdev (canonical limbs) -> v"""
        return self.plain(off) * self.Rinv % self.p

    def to_limbs(self, v):
        return [(v >> (self.lb * i)) & ((1 << self.lb) - 1) for i in range(self.nl)]

    def key_index(self, x):
        """sqrt_key's table index of the value x: a slice of the hash of the two low limbs of its Montgomery form"""
        l = self.to_limbs(x * self.R % self.p)
        w = (l[1] << 32) | l[0]
        return ((w * KEY_MUL & M64) >> self.kshift) & self.kmask

    def key(self, x):
        return self.keyt[self.key_index(x)]

    # ---- the kernels -----------------------------------------------------------------------------------------------------------------
    def pow_fixed(self, x, e, nbits):
        acc = x
        for i in range(nbits - 2, -1, -1):
            acc = acc * acc % self.p
            if (e >> i) & 1:
                acc = acc * x % self.p
        return acc

    def powers(self, A):
        """what sqrt_core computes before its look-ups: u, g, g^(2^8), g^(2^16), g^(2^24) (independent of `bug`: share them)"""
        p = self.p
        u = self.pow_fixed(A, self.e_sqrt, self.lay["bits_sqrt"])
        g = u * u * A % p
        out = [u, g]
        for _ in range(3):
            for _ in range(8):
                g = g * g % p
            out.append(g)
        return out

    def log(self, pw):
        p, negw = self.p, self.negw
        u, g, g8, g16, g24 = pw
        l0 = self.key(g24)
        h = g16 if self.bug == "no_correction" else g16 * negw[2][l0] % p
        l1 = self.key(h)
        l2 = self.key(g8 * negw[1][l0] * negw[2][l1] % p)
        l3 = self.key(g * negw[0][l0] * negw[1][l1] * negw[2][l2] % p)
        return l0 | l1 << 8 | l2 << 16 | l3 << 24

    def omega_pow(self, v):
        assert 0 <= v <= M32
        w = 1
        for m in range(4):
            w = w * self.posw[m][(v >> (8 * m)) & 255] % self.p
        return w

    def E(self, L):
        return (0 - (L >> 1)) & (M32 if self.bug == "wide_mask" else 0x7FFFFFFF)

    def sqrt(self, A, pw=None):
        """k_sqrt -> (L, root, has_root)"""
        if A == 0:
            return None, 0, 1
        pw = pw or self.powers(A)
        L = self.log(pw)
        if L & 1:
            return L, 0, 0
        return L, A * pw[0] * self.omega_pow(self.E(L)) % self.p, 1

    def finalize_s(self, A, pw=None):
        """k_randbit_finalize's s = x^-1 2^-1 of a square A that is not zero (None without a root)"""
        pw = pw or self.powers(A)
        L = self.log(pw)
        if L & 1:
            return None
        return pw[0] * self.omega_pow((0 - (L + self.E(L))) & M32) * self.half % self.p

    def inverse(self, x):
        return self.pow_fixed(x, self.e_inv, self.lay["bits_inv"])
