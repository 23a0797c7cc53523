"""The keys and messages of the signing latency path's tests (tests/test_sign_lat_host.py,
tests/test_gpu_sign_lat.py): the digit patterns of a key in base X = |x|, the curve parameter, which decide
what each of the four ladders of drand_amd/csrc/wsign.h does."""
from oracle import bls12381 as O

R = O.R
X = 0xD201000000010000
assert R == X ** 4 - X ** 2 + 1


def digits(k):
    """the four base-X digits of k mod r, least significant first"""
    k %= R
    return tuple((k // X ** j) % X for j in range(4))


# name -> key (any value below 2^256; the host reduces it mod r)
EDGE_KEYS = {
    "1": 1, "X": X, "X^2": X ** 2, "X^3": X ** 3,  # one digit equal to 1: one wave active, a ladder with no doubling
    "X-1": X - 1, "2^63": 2 ** 63,                  # a digit with bit 63 set
    "X^3-1": X ** 3 - 1,                            # three full digits
    "r-1": R - 1, "r-2": R - 2,
    "r+1": R + 1, "2^256-1": 2 ** 256 - 1,          # reduced by the host
}
ZERO_KEYS = {"0": 0, "r": R, "2r": 2 * R}           # the zero class: the point at infinity
INF_SIG = b"\xc0" + bytes(95)

assert digits(X - 1) == (X - 1, 0, 0, 0) and digits(2 ** 63) == (2 ** 63, 0, 0, 0) and X - 1 >= 2 ** 63
assert digits(X ** 3 - 1) == (X - 1, X - 1, X - 1, 0)
assert digits(R - 1) == (0, 0, X - 1, X - 1) and digits(R - 2) == (X - 1, X - 1, X - 2, X - 1)
assert [digits(X ** j) for j in range(4)] == [tuple(int(i == j) for i in range(4)) for j in range(4)]
assert all(digits(k) == (0, 0, 0, 0) for k in ZERO_KEYS.values()) and 2 * R < 2 ** 256
assert digits(R + 1) == (1, 0, 0, 0)

MSG_LENS = (0, 1, 32, 55, 56, 64, 300)


def msg_of(length, salt=0):
    """a fixed message of `length` bytes"""
    return bytes((7 * i + 13 * salt + length) & 0xFF for i in range(length))


MSG32 = msg_of(32)


def be32(k):
    return k.to_bytes(32, "big")
