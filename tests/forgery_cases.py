"""Forged verify rows, shared by the CPU tier (tests/test_verify_forgery_model.py) and the GPU tier
(tests/test_gpu_verify_forgery.py).  Pure Python, no device.

A verify row is (record, score, z_img, seed, pub_list), every part bytes.  One table (field_table) gives the offset and type of
every field for both R1CSProof layouts and any inner-product depth:

    compact    version byte 0 | A_I1 A_O1 S1 | T_1 T_3 T_4 T_5 T_6 | t_x t_x_blinding e_blinding | (L_j R_j) x lg_n | a b
    two-phase  version byte 1 | A_I1 A_O1 S1 A_I2 A_O2 S2 | the same from T_1 on

followed by the 4 + N commitments (V_0..V_3, C_0..C_{N-1}); the public inputs score, z_img, seed and pub_list are the other
parts of the row.

Two families of forgeries:

  cancelling sets   The inner-product scalars a and b never enter the transcript and the mega-check is linear in each, so a
                    valid row with a shifted by d has the residual d * X for a point X that depends on the row alone.  Copies of
                    one row shifted by d_1..d_k with sum d_i = 0 (mod l) are each invalid, and their residuals add up to the
                    identity: a verifier that adds the checks of a group with equal (or no) weights accepts all of them.
  field sweep       every field of the row under every mutation its type admits, swaps of fields, and fields transplanted from
                    another valid proof.  What each row's status is, the oracle decides; `differs` says whether the mutation
                    changed the value the verifier computes with (then the status must not be OK).
"""
import collections

from tests.test_oracle_kat import RFC9496_MULTIPLES

L = 2 ** 252 + 27742317777372353535851937790883648493
P = 2 ** 255 - 19
OK, VERIFY, FORMAT = 0, 1, 3
REC, SCORE, Z_IMG, SEED, PUB = range(5)

# kind: "vpoint" a point the verifier validates (identity refused) before it decodes it, "point" one it only decodes,
# "scalar" a proof scalar (canonical encodings only), "serde" a public scalar parsed canonical-only, "bits" a pub_list item
Field = collections.namedtuple("Field", "name kind part off")
Case = collections.namedtuple("Case", "label row differs")

b32 = lambda x: int(x).to_bytes(32, "little")
i32 = lambda b: int.from_bytes(b, "little")


def n_of(row):
    return len(row[PUB]) // 32


def field_table(row):
    """Every field of the row, in record order and then the public inputs."""
    rec, n = row[REC], n_of(row)
    plen = len(rec) - 32 * (4 + n)
    two = rec[0] == 1
    nel = (plen - 1) // 32
    lg = (nel - (6 if two else 3) - 5 - 3 - 2) // 2
    assert rec[0] in (0, 1) and plen == 1 + 32 * nel and lg >= 1 and nel == (6 if two else 3) + 10 + 2 * lg, "not a well-formed record"
    names = [("A_I1", "vpoint"), ("A_O1", "vpoint"), ("S1", "vpoint")]
    if two:
        names += [("A_I2", "point"), ("A_O2", "point"), ("S2", "point")]
    names += [("T_%d" % k, "vpoint") for k in (1, 3, 4, 5, 6)]
    names += [("t_x", "scalar"), ("t_x_blinding", "scalar"), ("e_blinding", "scalar")]
    for j in range(1, lg + 1):
        names += [("L_%d" % j, "vpoint"), ("R_%d" % j, "vpoint")]
    names += [("a", "scalar"), ("b", "scalar")]
    names += [("V_%d" % i, "point") for i in range(4)] + [("C_%d" % i, "point") for i in range(n)]
    out = [Field(nm, kind, REC, 1 + 32 * i) for i, (nm, kind) in enumerate(names)]
    assert out[-1].off + 32 == len(rec)
    out += [Field("score", "serde", SCORE, 0), Field("z_img", "serde", Z_IMG, 0), Field("seed", "serde", SEED, 0)]
    out += [Field("pub_%d" % i, "bits", PUB, 32 * i) for i in range(n)]
    return out


def fields_by_name(row):
    return {f.name: f for f in field_table(row)}


def get(row, f):
    return row[f.part][f.off:f.off + 32]


def put(row, f, value):
    assert len(value) == 32
    parts = list(row)
    parts[f.part] = parts[f.part][:f.off] + bytes(value) + parts[f.part][f.off + 32:]
    return tuple(parts)


def swap(row, f, g):
    return put(put(row, f, get(row, g)), g, get(row, f))


def join(row):
    return b"".join(row)


def two_phase(row):
    """The same proof in the two-phase layout: version byte 1, A_I2 = A_O2 = S2 = identity."""
    rec = row[REC]
    assert rec[0] == 0
    return (b"\x01" + rec[1:97] + bytes(96) + rec[97:],) + tuple(row[1:])


def bits_value(b):
    """What a pub_list item counts as: Scalar::from_bits clears bit 255, the arithmetic reduces mod l."""
    return (i32(b) & (2 ** 255 - 1)) % L


# ---- cancelling sets ------------------------------------------------------------------------------------------------------
def shifted(row, name, ds):
    """One copy of the row per d in ds, field `name` (a or b) replaced by value + d mod l."""
    f = fields_by_name(row)[name]
    v = i32(get(row, f))
    assert f.kind == "scalar" and v < L and all(d % L for d in ds)
    return [put(row, f, b32((v + d) % L)) for d in ds]


def cancelling_shifts(rnd):
    """{set name: d_1..d_k} with sum d_i = 0 (mod l) and no d_i = 0: a small pair, a 252-bit pair, the triple (d, d, -2d) and
    32 random shifts closed by the last (32 = the default aggregation group)."""
    big = (rnd.getrandbits(251) | 1 << 251) % L
    t = rnd.randrange(1, L)
    many = [rnd.randrange(1, L) for _ in range(31)]
    while sum(many) % L == 0:
        many[0] = rnd.randrange(1, L)
    many.append(-sum(many) % L)
    sets = {"pair_small": [3, L - 3], "pair_252": [big, L - big], "triple": [t, t, -2 * t % L], "set32": many}
    assert big.bit_length() == 252 and all(sum(ds) % L == 0 and all(d % L for d in ds) for ds in sets.values())
    return sets


def cancelling_sets(row, rnd, which=("pair_small", "pair_252", "triple", "set32")):
    """{"a:pair_small": [rows], ...} for the fields a and b."""
    out = {}
    for name in ("a", "b"):
        for k, ds in cancelling_shifts(rnd).items():
            if k in which:
                out["%s:%s" % (name, k)] = shifted(row, name, ds)
    return out


# ---- field sweep ------------------------------------------------------------------------------------------------------------
def _point_mutations(v, donor_v, other_valid):
    s = i32(v)
    neg = b32(P - s) if 0 < s < P else b32(1)  # the encoding of -s: a "negative" field element wherever s is a non-negative one
    return [("low_bit", bytes([v[0] ^ 1]) + v[1:]), ("high_bit", v[:31] + bytes([v[31] ^ 0x80])), ("identity", bytes(32)),
            ("ff", b"\xff" * 32), ("ge_p", b32(P + 1 + s % 18)), ("negative", neg), ("rfc_multiple", other_valid), ("donor", donor_v)]


def _scalar_mutations(v):
    return [("plus_1", b32((i32(v) + 1) % L)), ("zero", bytes(32)), ("l_minus_1", b32(L - 1)), ("l", b32(L)), ("all_ones", b"\xff" * 32)]


def sweep(row, donor, toggle):
    """Every mutation of every field of `row` (module doc).  donor: another valid row of the same N and layout; toggle: the index
    of the bid's own item in pub_list.  Rows that come out byte-identical to the original are dropped; labels are unique."""
    n = n_of(row)
    tab, dtab = field_table(row), fields_by_name(donor)
    byname = {f.name: f for f in tab}
    cases = []

    def add(label, new, differs=None):
        if new != row:
            cases.append(Case(label, new, (join(new) != join(row)) if differs is None else differs))

    for k, f in enumerate(tab):
        v, dv = get(row, f), get(donor, dtab[f.name])
        if f.kind in ("vpoint", "point"):
            other = bytes.fromhex(RFC9496_MULTIPLES[1 + k % 15])
            for tag, nv in _point_mutations(v, dv, other):
                add("%s:%s" % (f.name, tag), put(row, f, nv))
        elif f.kind == "scalar":
            for tag, nv in _scalar_mutations(v) + [("donor", dv)]:
                add("%s:%s" % (f.name, tag), put(row, f, nv))
        elif f.kind == "serde":
            for tag, nv in (("plus_1", b32((i32(v) + 1) % L)), ("plus_l", b32(i32(v) + L)), ("plus_2_255", b32(i32(v) + 2 ** 255)), ("donor", dv)):
                add("%s:%s" % (f.name, tag), put(row, f, nv))
        else:
            add("%s:plus_1" % f.name, put(row, f, b32((bits_value(v) + 1) % L)))
            # v + l: every item of a short list; of a long one the first, the bid's own and the last (one item is what is asked for)
            if n <= 8 or f.name in ("pub_0", "pub_%d" % toggle, "pub_%d" % (n - 1)):
                nv = b32(i32(v) + L)  # the same residue: the oracle decides, and accepts
                add("%s:plus_l" % f.name, put(row, f, nv), differs=bits_value(nv) != bits_value(v))
    lg = sum(1 for f in tab if f.name.startswith("L_"))
    pairs = [("L_%d" % j, "R_%d" % j) for j in range(1, lg + 1)] + [("L_1", "L_2"), ("T_3", "T_4"), ("V_0", "V_1"), ("V_3", "C_0"), ("a", "b")]
    if n >= 2:
        pairs += [("C_0", "C_%d" % (n - 1)), ("pub_%d" % toggle, "pub_%d" % ((toggle + 1) % n))]
    if n >= 3:
        others = [i for i in range(n) if i != toggle]
        pairs += [("pub_%d" % others[0], "pub_%d" % others[-1])]
    for x, y in pairs:
        new = swap(row, byname[x], byname[y])
        differs = None
        if byname[x].kind == "bits":
            differs = bits_value(get(row, byname[x])) != bits_value(get(row, byname[y]))
        add("swap:%s:%s" % (x, y), new, differs)
    assert len({c.label for c in cases}) == len(cases)
    return cases


def rejected_before_the_sum(row, status, decode, base=None):
    """Whether a non-OK row is already decided when an aggregated verifier adds up its group: format errors, validated points
    that are the identity encoding, and points that do not decode (`decode`: bytes -> point or None).  Such rows stay out of
    the group's sum and of the per-proof pass; every other bad row is only found by the (weighted) mega-check.  base: a valid
    row this one was made from -- only the fields that differ from it are looked at."""
    if status == FORMAT:
        return True
    if status == OK:
        return False
    for f in field_table(row):
        if base is not None and get(row, f) == get(base, f):
            continue
        if f.kind == "vpoint" and get(row, f) == bytes(32):
            return True
        if f.kind in ("vpoint", "point") and decode(get(row, f)) is None:
            return True
    return False


def expected_fallback(statuses, early, group):
    """How many proofs an aggregated call must check one by one: the members still OK after the front end (not `early`) of every
    group (cut by index) that holds a bad row the front end did not already reject."""
    if group <= 1:
        return 0
    total = 0
    for g0 in range(0, len(statuses), group):
        members = range(g0, min(len(statuses), g0 + group))
        if any(statuses[i] != OK and not early[i] for i in members):
            total += sum(1 for i in members if not early[i])
    return total
