"""The host side of pairwise-masked secure aggregation (Bonawitz et al., CCS 2017; the sparse mask graph of
Bell et al., CCS 2020): who masks with whom, the keys, the secret shares and what the server does to remove
the masks of a round. `fed_secagg` (worker/secagg_worker.py, algorithm/secagg_algorithm.py) runs it.

WHAT THIS IS NOT. Philox is not a cryptographic generator, the key agreement is Diffie-Hellman in a toy group
(the multiplicative group mod 2^127 − 1, generator 3, 64-bit exponents) and every "party" lives in one process.
Nothing here protects anybody's data. It reproduces what a deployment computes, moves and pays for.

Everything is python integers, keyed by (session seed, round): every rank computes the same values, nothing
is kept between rounds, and a resumed run repeats them.

Mask graph    over the round's SELECTED clients sorted by id (dropouts happen after the keys are agreed).
              degree 0 or ≥ n − 1: the complete graph; else an even d: position t is joined to t ± 1 … ± d/2
              (mod n). A client without partners (n = 1) masks nothing.
Secrets       client c draws a key-agreement secret s_c and a self-mask seed b_c, 64 bits each, from
              `ref.philox4x32` (its scalar form `philox4x32_int`) with counter (c, round, which, tag) under the
              session seed.
Key agreement pub_c = 3^s_c mod p; the pair key κ_ab = fold(pub_b^s_a) = fold(pub_a^s_b), fold(v) = (v ^ (v >> 64))
              mod 2^64. Computed once per pair and round: n · d / 2 modular powers are the whole cost (1.3e5 at
              512 clients on the complete graph), next to n for the public keys.
Masks         client c adds +w(κ_cj) for partners j > c, −w(κ_cj) for partners j < c and +w(b_c)
              (`ops.fl.secagg_mask_rows`); the pair masks cancel in the sum.
Shamir        c shares s_c and b_c among its d_c partners over the same prime, threshold t (`secagg_threshold`,
              default d_c // 2 + 1, 1 ≤ t ≤ d_c); the polynomial coefficients come from Philox too.
Recovery      S = the clients whose upload arrived, D = selected − S. For c ∈ S the server rebuilds b_c from
              the shares c's partners in S hold and removes +w(b_c); for x ∈ D with a partner in S it rebuilds
              s_x, derives κ_xj for every partner j ∈ S and removes the mask j added. It uses the REBUILT
              values only. Fewer than t shares for any of these: the round aborts.
Bytes         a client uploads 4 · num_params + 16 (public key) + 32 · d_c (two 16-B shares to each partner) +
              16 · d_c (one share returned per partner in the unmask step).
"""

from __future__ import annotations

import functools

from ..ops import ref

PRIME = 2 ** 127 - 1
GENERATOR = 3
TAG_SECRET = 0x53413032  # "SA02": per-client secrets
TAG_SHARE = 0x53413033  # "SA03": Shamir coefficients
_M64 = (1 << 64) - 1


def _words(seed: int, counter) -> list[int]:
    seed = int(seed) & _M64
    return list(ref.philox4x32_int(counter, (seed & 0xFFFFFFFF, seed >> 32)))


def draw64(seed: int, c0: int, c1: int, c2: int, tag: int) -> int:
    w = _words(seed, (c0, c1, c2, tag))
    return w[0] | (w[1] << 32)


def client_secrets(seed: int, rnd: int, client: int) -> tuple[int, int]:
    """(s_c, b_c): the key-agreement secret and the self-mask seed of `client` in round `rnd`."""
    return draw64(seed, client, rnd, 0, TAG_SECRET), draw64(seed, client, rnd, 1, TAG_SECRET)


def share_key(seed: int, rnd: int, client: int, which: int) -> int:
    """The 64-bit key of the Shamir polynomial of client's secret `which` (0: s_c, 1: b_c)."""
    return draw64(seed, client, rnd, 2 + which, TAG_SECRET)


def mask_graph(ids, degree: int) -> dict[int, list[int]]:
    """client id -> sorted partner ids over the sorted `ids`; see the module docstring. An odd degree (below
    n − 1) or a negative one raises ValueError."""
    ids = sorted(int(c) for c in ids)
    n, d = len(ids), int(degree)
    if len(set(ids)) != n:
        raise ValueError("secagg: duplicate client ids")
    if d < 0:
        raise ValueError(f"secagg_degree must be >= 0, got {d}")
    if d == 0 or d >= n - 1:
        return {c: [j for j in ids if j != c] for c in ids}
    if d % 2:
        raise ValueError(f"secagg_degree must be even (position t is joined to t +- 1 .. +- d/2), got {d}")
    return {c: sorted(ids[(t + k) % n] for k in range(-d // 2, d // 2 + 1) if k) for t, c in enumerate(ids)}


def public_key(secret: int) -> int:
    return pow(GENERATOR, secret, PRIME)


def pair_key(their_public: int, my_secret: int) -> int:
    v = pow(their_public, my_secret, PRIME)
    return (v ^ (v >> 64)) & _M64


def share(secret: int, xs, t: int, rng_key: int) -> list[tuple[int, int]]:
    """Shamir shares [(x, f(x))] of `secret` at the distinct non-zero points xs: f has degree t − 1, f(0) =
    secret, and coefficient j (1 ≤ j < t) is the 128 Philox bits of counter (j, 0, 0, TAG_SHARE) under
    `rng_key`, reduced mod p. Any t shares give the secret back; fewer say nothing about it."""
    xs = [int(x) for x in xs]
    if not 1 <= t <= len(xs):
        raise ValueError(f"secagg: threshold {t} outside [1, {len(xs)}]")
    if len(set(xs)) != len(xs) or any(not 0 < x < PRIME for x in xs):
        raise ValueError("secagg: share points must be distinct and non-zero")
    coef = [int(secret) % PRIME]
    for j in range(1, t):
        w = _words(rng_key, (j, 0, 0, TAG_SHARE))
        coef.append((w[0] | (w[1] << 32) | (w[2] << 64) | (w[3] << 96)) % PRIME)
    out = []
    for x in xs:
        y = 0
        for a in reversed(coef):  # Horner
            y = (y * x + a) % PRIME
        out.append((x, y))
    return out


def reconstruct(points) -> int:
    """f(0) by Lagrange interpolation through `points` [(x, y)] over the prime field."""
    total = 0
    for i, (xi, yi) in enumerate(points):
        num = den = 1
        for j, (xj, _) in enumerate(points):
            if i != j:
                num = num * (-xj) % PRIME
                den = den * (xi - xj) % PRIME
        total = (total + yi * num * pow(den, -1, PRIME)) % PRIME
    return total


class RoundProtocol:
    """One round of the protocol over the selected clients. `shares[c][j]` = [share of s_c, share of b_c] held
    by partner j (plain lists: a test corrupts one to show that recovery uses what it rebuilds)."""

    def __init__(self, seed: int, rnd: int, selected, degree: int = 0, threshold: int | None = None):
        self.seed, self.round = int(seed), int(rnd)
        self.ids = sorted(int(c) for c in selected)
        self.partners = mask_graph(self.ids, degree)
        self.threshold = None if threshold is None else int(threshold)
        for c in self.ids:
            d = len(self.partners[c])
            if d and not 1 <= self.threshold_of(c) <= d:
                raise ValueError(f"secagg_threshold {self.threshold} outside [1, {d}] (the degree of client {c})")
        self.secrets = {c: client_secrets(self.seed, self.round, c) for c in self.ids}
        self.public = {c: public_key(self.secrets[c][0]) for c in self.ids}
        self.pair_keys: dict[tuple[int, int], int] = {}  # (a, b), a < b: from a's side, once per pair
        for a in self.ids:
            for b in self.partners[a]:
                if a < b:
                    self.pair_keys[(a, b)] = pair_key(self.public[b], self.secrets[a][0])
        self._shares: dict[int, dict[int, list[tuple[int, int]]]] = {}

    def degree_of(self, c: int) -> int:
        return len(self.partners[c])

    def threshold_of(self, c: int) -> int:
        return self.degree_of(c) // 2 + 1 if self.threshold is None else self.threshold

    def shares_of(self, c: int) -> dict[int, list[tuple[int, int]]]:
        """partner id -> [share of s_c, share of b_c]; the share point of partner j is j + 1."""
        if c not in self._shares:
            ps = self.partners[c]
            xs, t = [j + 1 for j in ps], self.threshold_of(c)
            per = [share(self.secrets[c][which], xs, t, share_key(self.seed, self.round, c, which)) for which in (0, 1)]
            self._shares[c] = {j: [per[0][i], per[1][i]] for i, j in enumerate(ps)}
        return self._shares[c]

    def client_entries(self, c: int) -> list[tuple[int, int]]:
        """[(κ, sign)] of client c's upload: +w(κ_cj) for partners j > c, −w(κ_cj) for j < c, +w(b_c)."""
        ps = self.partners[c]
        if not ps:
            return []
        out = [(self.pair_keys[(min(c, j), max(c, j))], 1 if j > c else -1) for j in ps]
        out.append((self.secrets[c][1], 1))
        return out

    def entry_table(self, clients) -> tuple[list[int], list[int], list[int]]:
        """(offsets, keys, signs) of `ops.fl.secagg_mask_rows` for the rows of `clients`, in their order."""
        offsets, keys, signs = [0], [], []
        for c in clients:
            for k, s in self.client_entries(c):
                keys.append(k)
                signs.append(s)
            offsets.append(len(keys))
        return offsets, keys, signs

    def row_bytes(self, c: int, num_params: int) -> int:
        d = self.degree_of(c)
        return 4 * int(num_params) + 16 + 32 * d + 16 * d

    def dropped_bytes(self, c: int) -> int:
        """What a client that dropped had already sent: its public key and the shares to its partners."""
        return 16 + 32 * self.degree_of(c)

    def _rebuild(self, c: int, which: int, holders: list[int]) -> int | None:
        t = self.threshold_of(c)
        if len(holders) < t:
            return None
        held = self.shares_of(c)
        return reconstruct([held[j][which] for j in holders[:t]]) & _M64

    def recover(self, reporting) -> tuple[list[int], list[int], bool]:
        """(keys, signs, aborted): the flat entry list of `ops.fl.ring_unmask` for the reporting set, from
        rebuilt secrets only. aborted: some secret had fewer than t shares among the reporting clients (the
        lists are then empty)."""
        S = set(int(c) for c in reporting)
        if not S <= set(self.ids):
            raise ValueError(f"secagg: uploads from clients outside the round's selection: {sorted(S - set(self.ids))}")
        keys, signs = [], []
        for c in self.ids:
            holders = [j for j in self.partners[c] if j in S]
            if c in S:
                if not self.partners[c]:
                    continue  # (no partners: nothing was masked)
                b = self._rebuild(c, 1, holders)
                if b is None:
                    return [], [], True
                keys.append(b)
                signs.append(1)
            elif holders:
                s = self._rebuild(c, 0, holders)
                if s is None:
                    return [], [], True
                for j in holders:  # the mask j added for its partner c: + if c > j
                    keys.append(pair_key(self.public[j], s))
                    signs.append(1 if c > j else -1)
        return keys, signs, False


@functools.lru_cache(maxsize=4)
def _cached(seed: int, rnd: int, selected: tuple, degree: int, threshold) -> RoundProtocol:
    return RoundProtocol(seed, rnd, selected, degree, threshold)


def round_protocol(seed: int, rnd: int, selected, degree: int = 0, threshold: int | None = None) -> RoundProtocol:
    """The round's protocol object; the client side and the server replica of one process share it (the
    server still uses only what it rebuilds from shares)."""
    return _cached(int(seed), int(rnd), tuple(sorted(int(c) for c in selected)), int(degree),
                   None if threshold is None else int(threshold))
