"""Witness cases for checked proving (tests/test_prove_check_host.py, tests/test_gpu_prove_check.py): honest rows, each circuit
relation broken on its own, and the encodings the circuit accepts although the scalars look wrong (a wrong y, a list item
encoded as x + l or with bit 255 set, the toggle on a second copy of x).  Witnesses come from the C oracle (oc.witness)."""
import hashlib

from oracle.ref_py import ristretto as rs

L = rs.L


def b32(x):
    return (x % (1 << 256)).to_bytes(32, "little")


def sc(b):
    return int.from_bytes(b, "little")


def _stream(seed, i, tag):
    return hashlib.sha512(b"bbp-check-v1" + seed.to_bytes(8, "little") + i.to_bytes(8, "little") + tag).digest()


def honest(oc, seed, N, toggle=None):
    """(fields, pub_list, toggle): fields = [d, k, y, y_inv, q, z_img, seed] as ints, pub_list as a list of 32-byte encodings."""
    d = sc(_stream(seed, 0, b"d")[:8])
    k = sc(rs.sc_bytes(rs.sc_wide(_stream(seed, 0, b"k"))))
    sd = sc(rs.sc_bytes(rs.sc_wide(_stream(seed, 0, b"seed"))))
    w = oc.witness(b32(d) + b32(k) + b32(sd))
    m, x, y, yi, q, z = (sc(w[32 * j:32 * j + 32]) for j in range(6))
    t = seed % N if toggle is None else toggle
    pub = [rs.sc_bytes(rs.sc_wide(_stream(seed, j, b"pub"))) for j in range(N)]
    pub[t] = b32(x)
    return dict(f=[d, k, y, yi, q, z, sd], pub=pub, toggle=t, x=x)


def row(c):
    """bbp_prove_batch input row: scalars7 || pub_list || toggle (u64 LE)."""
    return b"".join(b32(v) for v in c["f"]) + b"".join(c["pub"]) + int(c["toggle"]).to_bytes(8, "little")


def scalars7(c):
    return b"".join(b32(v) for v in c["f"])


def entropy(seed, N):
    return b"".join(rs.sc_bytes(rs.sc_wide(_stream(seed, j, b"ent"))) for j in range(4 + N)) + _stream(seed, 0, b"entseed")[:32]


def _edit(c, **kw):
    e = dict(f=list(c["f"]), pub=list(c["pub"]), toggle=c["toggle"], x=c["x"])
    e.update(kw)
    return e


D, K, Y, YI, Q, Z, SEED = range(7)


def variants(oc, seed, N):
    """[(name, case, satisfied)] around one honest witness of list length N."""
    c = honest(oc, seed, N)
    f, x, t = c["f"], c["x"], c["toggle"]
    out = [("honest", c, True)]

    def with_f(i, v):
        g = list(f)
        g[i] = v % L
        return g
    out.append(("y_only_wrong", _edit(c, f=with_f(Y, f[Y] + 5)), True))               # y is committed, never constrained
    pub = list(c["pub"])
    pub[t] = b32(x + L)
    out.append(("item_x_plus_l", _edit(c, pub=pub), True))                              # Scalar::from_bits, used mod l
    pub = list(c["pub"])
    pub[t] = b32(x + (1 << 255))
    out.append(("item_bit255", _edit(c, pub=pub), True))                                # bit 255 cleared by from_bits
    pub = list(c["pub"])
    pub[t] = b32(x + 1)
    out.append(("list_wrong", _edit(c, pub=pub), False))
    out.append(("z_img_wrong", _edit(c, f=with_f(Z, f[Z] + 1)), False))
    yi2 = (f[YI] + 1) % L
    g = with_f(YI, yi2)
    g[Q] = f[D] * yi2 % L                                                               # q still d * y_inv: only y * y_inv = 1 breaks
    out.append(("y_inv_wrong", _edit(c, f=g), False))
    out.append(("q_wrong", _edit(c, f=with_f(Q, f[Q] + 1)), False))
    out.append(("k_wrong", _edit(c, f=with_f(K, f[K] + 1)), False))                     # m moves: x and z_img break
    out.append(("d_wrong", _edit(c, f=with_f(D, f[D] + 1)), False))                     # x and q break
    out.append(("seed_wrong", _edit(c, f=with_f(SEED, f[SEED] + 1)), False))           # z_img and the score break
    out.append(("toggle_is_n", _edit(c, toggle=N), False))
    if N > 1:
        other = (t + 1) % N
        pub = list(c["pub"])
        pub[other] = b32(x)
        out.append(("toggle_on_second_copy", _edit(c, pub=pub, toggle=other), True))
        pub = list(c["pub"])
        out.append(("toggle_on_other_item", _edit(c, toggle=other), False))
    return out
