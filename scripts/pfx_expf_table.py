"""Generator of the constants of pcl_feature_extraction_amd/csrc/pfx_expf.h: the 32 table entries
2^(i/32) and the reduction and polynomial constants, each correctly rounded to an IEEE double from a
50-digit decimal evaluation (the standard library's `decimal` only).  Prints the C++ initialisers; the
header holds a copy of this output, and tests/test_pfx_expf.py compares the two.

    python scripts/pfx_expf_table.py
"""
import decimal
import fractions
import struct

N = 32          # table entries: 2^(i/N)
DIGITS = 50     # working precision; a double needs 17


def to_double(v):
    """The IEEE double nearest to the Decimal v (exact rational -> float is correctly rounded)."""
    return float(fractions.Fraction(v))


def bits(d):
    return struct.unpack("<Q", struct.pack("<d", d))[0]


def constants():
    decimal.getcontext().prec = DIGITS
    ln2 = decimal.Decimal(2).ln()
    # T[i] = the bits of 2^(i/N) less i << (52 - 5): adding k << 47 for k = N e + i then sets the
    # exponent to e and leaves the mantissa of 2^(i/N)
    table = [bits(to_double((ln2 * i / N).exp())) - (i << 47) for i in range(N)]
    step = ln2 / N   # 2^(r/N) = exp(r step) = 1 + step r + step^2/2 r^2 + step^3/6 r^3 + ...
    return dict(table=table, inv_ln2_n=to_double(N / ln2), c1=to_double(step), c2=to_double(step * step / 2),
                c3=to_double(step * step * step / 6))


def render(c):
    rows = ["    " + ", ".join("0x%016xull" % v for v in c["table"][i:i + 4]) + "," for i in range(0, N, 4)]
    lines = ["// 2^(i/32), i = 0 .. 31, as bits less i << 47", *rows]
    for name in ("inv_ln2_n", "c1", "c2", "c3"):
        lines.append("%-9s = %s  (0x%016x)" % (name, c[name].hex(), bits(c[name])))
    return "\n".join(lines)


if __name__ == "__main__":
    print(render(constants()))
