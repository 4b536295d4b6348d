"""Bases of mixed limb sizes for the limb-aware libraries (tests/test_gpu_bases.py): plain data and
arithmetic, no GPU, and no library load at import.  tests/test_basis_cases.py holds every literal
to the walk that defines it.

Every prime is = 1 mod 2^17, so a profile serves every n <= 65536.  An anchor ("down", e) is the
first primes of that form below 2^e, walking down; ("up", e) the first at or above 2^e, walking up
(("up", 0): the smallest such primes at all).  A profile takes its limbs from the anchors in the
order its table gives, which is not sorted: the contexts of the tests are created in that order.

    bottom64     Q: 2^32 up                                  P: the next K above those
    chain64      Q: 2^60 down, then in turn 2^40 up, 2^50    P: in turn 2^62 down, 2^61 down
                 down, 2^45 up, 2^33 up, repeating              (above every q)
    chain64_rev  Q: 2^62 down                                P: 2^32 up (below every q: ModDown
                                                                from the smallest limbs into the
                                                                largest)
    chain32      Q: 2^31 down, then in turn 2^25 up, 2^28    P: in turn 2^31 down after q_0,
                 down, the smallest primes, repeating           2^30 down
    chain32_rev  Q: 2^31 down                                P: the smallest primes

The word classes are the libraries': 32-bit words hold moduli below 2^31, 64-bit words moduli in
[2^32, 2^62)."""

STEP = 1 << 17
PER_ANCHOR = 9                 # literals kept per anchor; basis() asserts it never needs more
CLASS = {32: (2, 1 << 31), 64: (1 << 32, 1 << 62)}          # [lo, hi) of a modulus

ANCHORS = {
    ("down", 62): (4611686018425815041, 4611686018423062529, 4611686018422669313,
                   4611686018416115713, 4611686018408120321, 4611686018406940673,
                   4611686018406678529, 4611686018405498881, 4611686018405367809),
    ("down", 61): (2305843009211596801, 2305843009210023937, 2305843009208713217,
                   2305843009202159617, 2305843009201242113, 2305843009200586753,
                   2305843009196916737, 2305843009195868161, 2305843009195343873),
    ("down", 60): (1152921504606584833, 1152921504598720513, 1152921504597016577,
                   1152921504595968001, 1152921504592822273, 1152921504592429057,
                   1152921504589938689, 1152921504586530817, 1152921504583647233),
    ("down", 50): (1125899903827969, 1125899902124033, 1125899887312897, 1125899886395393,
                   1125899885740033, 1125899884167169, 1125899884036097, 1125899883642881,
                   1125899883380737),
    ("up", 45): (35184372744193, 35184373006337, 35184376545281, 35184377331713, 35184378511361,
                 35184379035649, 35184380870657, 35184382967809, 35184383229953),
    ("up", 40): (1099512938497, 1099515691009, 1099516870657, 1099521458177, 1099522375681,
                 1099523555329, 1099525128193, 1099526176769, 1099529060353),
    ("up", 33): (8590458881, 8590983169, 8592949249, 8594784257, 8604352513, 8604614657,
                 8605532161, 8606187521, 8608153601),
    ("up", 32): (4296540161, 4298506241, 4299685889, 4300210177, 4300865537, 4301651969,
                 4302176257, 4302569473, 4304535553),
    ("down", 31): (2147352577, 2146959361, 2146041857, 2144468993, 2142502913, 2135818241,
                   2135162881, 2135031809, 2134638593),
    ("down", 30): (1073479681, 1071513601, 1070727169, 1068236801, 1065484289, 1064697857,
                   1062862849, 1062469633, 1060765697),
    ("down", 28): (268042241, 265420801, 264634369, 263454721, 263323649, 261881857, 261488641,
                   260702209, 260571137),
    ("up", 25): (35389441, 36175873, 37224449, 38535169, 39714817, 40370177, 41680897, 42729473,
                 44433409),
    ("up", 0): (786433, 1179649, 2752513, 5767169, 6684673, 6946817, 7340033, 8257537, 8519681),
}

# profile -> (word bits, the anchor of q_0 or None, the anchors Q cycles through after it,
#             the anchors P cycles through)
PROFILES = {
    "bottom64": (64, None, (("up", 32),), (("up", 32),)),
    "chain64": (64, ("down", 60), (("up", 40), ("down", 50), ("up", 45), ("up", 33)),
                (("down", 62), ("down", 61))),
    "chain64_rev": (64, None, (("down", 62),), (("up", 32),)),
    "chain32": (32, ("down", 31), (("up", 25), ("down", 28), ("up", 0)),
                (("down", 31), ("down", 30))),
    "chain32_rev": (32, None, (("down", 31),), (("up", 0),)),
}
OF_BITS = {bits: tuple(name for name, v in PROFILES.items() if v[0] == bits) for bits in (32, 64)}
CHAINS = {32: ("chain32", "chain32_rev"), 64: ("chain64", "chain64_rev")}
MAX_SHAPE = (5, 5)             # the largest L and the largest K any test asks of a profile,
MAX_LIMBS = 9                  # and the largest L + K


def bits_of(profile):
    return PROFILES[profile][0]


def walk(anchor, count, is_prime):
    """The first `count` primes = 1 mod 2^17 of an anchor, by the walk that defines it."""
    way, e = anchor
    a = (1 << e) if e else 2
    q = (a - 2) // STEP * STEP + 1 if way == "down" else -(-(a - 1) // STEP) * STEP + 1
    out = []
    while len(out) < count:
        assert q > 2
        if (way == "down" or q >= a) and is_prime(q):
            out.append(q)
        q += -STEP if way == "down" else STEP
    return tuple(out)


def basis(profile, L, K):
    """(q, p): the profile's L limbs of Q and K limbs of P, in the order its table gives.  Each
    anchor hands out its primes in turn, to Q first and then to P."""
    _, first, q_cycle, p_cycle = PROFILES[profile]
    taken = {}

    def take(anchor):
        i = taken.get(anchor, 0)
        assert i < PER_ANCHOR, (profile, L, K, anchor)
        taken[anchor] = i + 1
        return ANCHORS[anchor][i]

    q = [take(first)] if first else []
    q += [take(q_cycle[i % len(q_cycle)]) for i in range(L - len(q))]
    p = [take(p_cycle[j % len(p_cycle)]) for j in range(K)]
    return tuple(q), tuple(p)
