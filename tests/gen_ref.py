"""A plain-Python restatement of the reference's Oxford GEN reader, one cell at a time: gnrParseGEN (src/ConvToGDS.cpp:1015-1157),
CReadLine::GetCell splitting by space and tab (:123-179), getInt32 (:467-503), getFloat (:506-532), the error text of
COREARRAY_TRY_END (:260-277), and the sample file as R/Conversion.R:849-858 reads it.  Numbers go through the C library's own
strtof / strtod / strtol by ctypes -- never through float() or np.float32(str), which round twice.  Also: the kernel's rounding
rule restated (round_rule), what its grammar flags (predict_flags), and a generator of GEN text."""
import ctypes
import ctypes.util
import gzip
import re

import numpy as np

_libc = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libc.strtof.restype, _libc.strtof.argtypes = ctypes.c_float, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
_libc.strtod.restype, _libc.strtod.argtypes = ctypes.c_double, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
_libc.strtol.restype, _libc.strtol.argtypes = ctypes.c_long, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.c_int]
_libm.fma.restype, _libm.fma.argtypes = ctypes.c_double, [ctypes.c_double] * 3

SPACE = b" \t\n\v\f\r"                                     # isspace in the C locale
NA_INTEGER = -2147483648
FLAG_BYTE, FLAG_DOT, FLAG_DIGITS, FLAG_LONG, FLAG_EMPTY, FLAG_COUNT = 1, 2, 4, 8, 16, 32
HALO = 64
MIDPOINTS = ("0.542436033487320", "0.654068261384964", "16777217")


def _c_call(fn, s, *more):
    buf = ctypes.create_string_buffer(bytes(s))            # NUL-terminated
    end = ctypes.c_void_p()
    v = fn(ctypes.addressof(buf), ctypes.byref(end), *more)
    return v, end.value - ctypes.addressof(buf)


def strtof(s):
    """(the float strtof gives, widened exactly to a Python float; bytes consumed)"""
    return _c_call(_libc.strtof, s)


def strtod(s):
    return _c_call(_libc.strtod, s)


def strtol(s):
    return _c_call(_libc.strtol, s, 10)


class GenError(ValueError):
    """an error of the reference's parser: .message is its text, .column / .cell what COREARRAY_TRY_END appends"""

    def __init__(self, message, column=0, cell=b""):
        ValueError.__init__(self, message)
        self.message, self.column, self.cell = message, column, cell


def _skip(s):
    i = 0
    while i < len(s) and s[i] in SPACE:
        i += 1
    return s[i:]


def _short(p):
    p = p.decode("latin1")
    return p if len(p) <= 16 else p[:16] + "..."


def get_float(txt):
    """getFloat(txt, RaiseError = true): (double) strtof; NaN for a cell where nothing converts and that starts with '.'"""
    p = _skip(txt)
    v, used = strtof(p)
    if used == 0:
        if p[:1] != b".":
            raise GenError("Invalid float conversion \"%s\"." % _short(p))
        return float("nan")
    p = _skip(p[used:])
    if p:
        raise GenError("Invalid float conversion \"%s\"." % _short(p))
    return v


def get_int32(txt):
    p = _skip(txt)
    v, used = strtol(p)
    if used == 0:
        if p[:1] != b".":
            raise GenError("Invalid integer conversion \"%s\"." % _short(p))
        return NA_INTEGER
    if v < -(1 << 31) or v > (1 << 31) - 1:
        raise GenError("Invalid integer conversion \"%s\"." % _short(p))
    rest = _skip(p[used:])
    if rest:
        raise GenError("Invalid integer conversion \"%s\"." % _short(rest))
    return v


class Line:
    """CReadLine over one line held as a C string, SplitBySpaceTab"""

    def __init__(self, line):
        z = line.find(b"\0")
        self.s = line if z < 0 else line[:z]
        self.p, self.column = 0, 0

    def get_cell(self, last):
        s, b = self.s, self.p
        e = b
        while e < len(s) and s[e] not in b"\t ":
            e += 1
        self.column += 1
        if b == e and e == len(s):
            raise GenError("fewer columns than what expected.")
        p = e
        if last:
            while p < len(s) and s[p] == 0x20:
                p += 1
            if p < len(s):
                raise GenError("more columns than what expected.")
        elif p < len(s) and s[p] == 0x09:
            p += 1
        else:
            while p < len(s) and s[p] == 0x20:
                p += 1
        self.p = p
        if e > b + 1 and ((s[b] == 0x22 and s[e - 1] == 0x22) or (s[b] == 0x27 and s[e - 1] == 0x27)):
            b, e = b + 1, e - 1
        return s[b:e]


def call(p_aa, p_ab, p_bb, thr):
    """src/ConvToGDS.cpp:1134-1145, branch for branch"""
    if p_aa >= p_ab:
        if p_aa >= p_bb:
            return 2 if p_aa >= thr else 3
        else:
            return 0 if p_bb >= thr else 3
    else:
        if p_ab >= p_bb:
            return 1 if p_ab >= thr else 3
        else:
            return 0 if p_bb >= thr else 3


def parse_line(line, n_samp, thr=0.9, cell=b""):
    """one line (bytes without the '\\n') as the loop body of gnrParseGEN: ((snp id, rs id, position, "A/B"), codes uint8, the
    `cell` variable after the line).  `cell`: that variable before the line.  GenError carries column and cell."""
    rl = Line(line)
    try:
        cell = rl.get_cell(False)
        snp = cell
        cell = rl.get_cell(False)
        rs = cell
        cell = rl.get_cell(False)
        pos = get_int32(cell)
        allele = rl.get_cell(False) + b"/" + rl.get_cell(False)                  # AlleleA, AlleleB: not `cell`
        codes = np.empty(n_samp, np.uint8)
        for j in range(n_samp):
            pr = []
            for q in range(3):
                cell = rl.get_cell(q == 2 and j >= n_samp - 1)
                pr.append(get_float(cell))
            codes[j] = call(pr[0], pr[1], pr[2], thr)
    except GenError as err:
        raise GenError(err.message, rl.column, cell)
    return (snp.decode("latin1"), rs.decode("latin1"), pos, allele.decode("latin1")), codes, cell


def split_lines(text):
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return lines


def parse_text(text, n_samp, thr=0.9, path="x.gen"):
    """a whole .gen file: (list of heads, codes uint8 [n_lines][n_samp]); ValueError with the text of COREARRAY_TRY_END"""
    heads, rows, cell = [], [], b""
    for k, line in enumerate(split_lines(text)):
        try:
            head, codes, cell = parse_line(line, n_samp, thr, cell)
        except GenError as err:
            raise ValueError("%s\nFILE: %s\nLINE: %d, COLUMN: %d, %s\n" % (err.message, path, k + 1, err.column, err.cell.decode("latin1")))
        heads.append(head)
        rows.append(codes)
    return heads, (np.stack(rows) if rows else np.zeros((0, n_samp), np.uint8))


def pack_rows(codes):
    """uint8 [L][N] -> PACKED2 rows with padding codes 0"""
    L, N = codes.shape
    g = np.zeros((L, (N + 3) // 4 * 4), np.uint8)
    g[:, :N] = codes
    g = g.reshape(L, -1, 4)
    return (g[:, :, 0] | (g[:, :, 1] << 2) | (g[:, :, 2] << 4) | (g[:, :, 3] << 6)).astype(np.uint8)


def read_sample(path, version=">=2.0"):
    """(names, rows of text) of a sample file: read.table(header = TRUE), with ">=2.0" the line of column types skipped"""
    op = gzip.open if str(path).endswith(".gz") else open
    with op(path, "rb") as f:
        lines = [ln.decode("latin1").split() for ln in f.read().split(b"\n")]
    lines = [t for t in lines if t]
    return lines[0], lines[2 if version == ">=2.0" else 1:]


# ---- the kernel's rule for a number, restated ---------------------------------------------------------------------------------------------
_TOKEN = re.compile(rb"(\d+)(?:\.(\d*))?$|\.(\d+)$")


def round_rule(tok):
    """the float (widened) of a fast-grammar token by the rule of DESIGN section 28: m and k, d = m / 10^k in fp64, the low 29
    bits of d against 0x10000000, the sign of fma(d, 10^k, -m) at the midpoint.  None when the token is outside the grammar."""
    mt = _TOKEN.match(tok)
    if not mt:
        return None
    whole, frac = (mt.group(1), mt.group(2) or b"") if mt.group(1) is not None else (b"", mt.group(3))
    digits = (whole + frac).lstrip(b"0")
    k = len(frac)
    if len(digits) > 15 or k > 22:
        return None
    m = int(digits) if digits else 0
    if m == 0:
        return 0.0
    p = float(10 ** k)                                     # exact up to 10^22
    d = float(m) / p
    bits = int(np.float64(d).view(np.uint64))
    low = bits & 0x1FFFFFFF
    up = low > 0x10000000
    if low == 0x10000000:
        r = _libm.fma(d, p, -float(m))
        up = r < 0 or (r == 0 and bool(bits & 0x20000000))
    bits = (bits & ~0x1FFFFFFF) + (0x20000000 if up else 0)
    return float(np.uint64(bits).view(np.float64))


def float_of_double(d):
    """(float) d, widened"""
    return float(np.float32(d))


def double_rounding_cases(rng, want, tries=200000):
    """decimal strings of 15 significant digits s with strtof(s) != (float) strtod(s): the double nearest s is exactly the midpoint
    of two floats and s is not.  Found by search around the midpoints of random floats in [0.5, 1)."""
    out = []
    for _ in range(tries):
        f = np.float32(0.5 + 0.5 * rng.random())
        mid = (float(f) + float(np.nextafter(f, np.float32(2)))) / 2            # exact in fp64
        s = ("%.15f" % mid).encode()
        a, b = strtof(s)[0], float_of_double(strtod(s)[0])
        if a != b:
            out.append(s.decode())
            if len(out) >= want:
                break
    return out


# ---- what the kernel's grammar flags -------------------------------------------------------------------------------------------------------
def predict_flags(cells, n_samp):
    """the flags of snpgpu_gen_genotypes for the bytes of a line from its sixth column on (include/snpgpu.h section 1p), and the
    number of tokens"""
    fl, n = 0, len(cells)
    for p in range(n):
        c = cells[p]
        if c not in b" \t":
            continue
        nxt = cells[p + 1] if p + 1 < n else None
        if p == 0:
            fl |= FLAG_EMPTY
        if c == 9 and (nxt is None or nxt in b" \t"):
            fl |= FLAG_EMPTY
        if c == 0x20 and nxt == 9:
            fl |= FLAG_EMPTY
    toks = [t for t in re.split(rb"[ \t]+", cells) if t]
    for t in toks:
        if len(t) > HALO:
            fl |= FLAG_LONG
            t = t[:HALO]
        point, digit, nd, k, lead = False, False, 0, 0, True
        for c in t:
            if 0x30 <= c <= 0x39:
                digit = True
                k += point
                lead = lead and c == 0x30
                nd += not lead
            elif c == 0x2E and not point:
                point = True
            else:
                fl |= FLAG_BYTE
        if not digit:
            fl |= FLAG_DOT
        if nd > 15 or k > 22:
            fl |= FLAG_DIGITS
    if len(toks) != 3 * n_samp:
        fl |= FLAG_COUNT
    return fl, len(toks)


# ---- GEN text ----------------------------------------------------------------------------------------------------------------------------------
K22 = "0.0000000000000000000001"
FORMS = ("0", "1", "1.", ".5", "00.250", "digits", "k22")


def token(rng, form):
    if form == "digits":                                   # 3 ... 15 significant digits, mostly near the default threshold
        n = int(rng.integers(3, 16))
        lead = "9" if rng.random() < 0.6 else str(int(rng.integers(1, 10)))
        return "0." + lead + "".join(str(int(x)) for x in rng.integers(0, 10, n - 1))
    return K22 if form == "k22" else form


def make_line(rng, n_samp, forms=FORMS, sep=" ", snp="snp", rs="rs1", pos=100, alleles=("A", "G"), tokens=None, head_sep=None):
    """one line without its end: five leading columns, then 3 n_samp tokens.  sep: " ", "\\t", or "runs" (1 ... 3 spaces);
    head_sep: the separator between the leading columns when it is another one (a tab lets a leading cell be empty)"""
    def s():
        return " " * int(rng.integers(1, 4)) if sep == "runs" else sep

    def h():
        return head_sep if head_sep is not None else s()
    toks = tokens if tokens is not None else [token(rng, forms[int(rng.integers(len(forms)))]) for _ in range(3 * n_samp)]
    out = [snp, h(), rs, h(), str(pos), h(), alleles[0], h(), alleles[1]]
    for t in toks:
        out += [s(), t]
    return "".join(out).encode("latin1")


def make_text(rng, n_samp, n_lines, forms=FORMS, sep=" ", newline=b"\n", final_newline=True, rs_len=None, head_sep=None):
    lines = [make_line(rng, n_samp, forms, sep, snp="snp%d" % (i + 1), rs=("r" * rs_len if rs_len is not None else "rs%d" % (i + 1)),
                       pos=1000 + i, alleles=("ACGT"[i % 4], "CGTA"[i % 4]), head_sep=head_sep) for i in range(n_lines)]
    return newline.join(lines) + (newline if final_newline else b"")


def write_sample(path, ids, version=">=2.0", extra=None):
    """a sample file: ID_1 ID_2 missing [+ extra columns {name: values}]"""
    extra = extra or {}
    with open(path, "w") as f:
        f.write(" ".join(["ID_1", "ID_2", "missing"] + list(extra)) + "\n")
        if version == ">=2.0":
            f.write(" ".join(["0", "0", "0"] + ["D"] * len(extra)) + "\n")
        for i, s in enumerate(ids):
            f.write(" ".join([str(s), str(s), "0"] + [str(v[i]) for v in extra.values()]) + "\n")
