"""VCF text for the tests: data lines built from a matrix of dosage codes, every cell in a randomly chosen regular style
(phased and unphased, haploid to triploid, the '.' forms, multi-digit allele indices, 0 to 3 further FORMAT sub-fields), with
hooks to plant irregular cells and to control every byte of a line.  Nothing here parses: what a text means is vcf_ref's to say."""
import numpy as np

HEADER = "##fileformat=VCFv4.1\n##source=vcf_cases\n"
ALT_POOL = ["C", "G", "T", "AC", "AG", "AT", "ACG", "ACT", "AGT", "CGT", "ACGT"]


def gt_of_code(rng, code, num_allele):
    """a regular GT whose dosage of allele 0 is `code` (3: a missing allele); num_allele >= 2"""
    assert num_allele >= 2 and 0 <= code <= 3
    ploidy = int(rng.choice([1, 2, 2, 2, 3]))
    other = lambda: str(int(rng.integers(1, num_allele)))                      # noqa: E731
    if code == 3:
        al = ["." if rng.random() < 0.6 else str(int(rng.integers(0, num_allele))) for _ in range(ploidy)]
        al[int(rng.integers(0, ploidy))] = "."
    else:
        if code == 2:
            ploidy = int(rng.choice([2, 2, 3]))
            k = ploidy if rng.random() < 0.6 else 2                               # three copies still give 2
        else:
            k = code
            ploidy = max(ploidy, k)
        al = ["0"] * k + [other() for _ in range(ploidy - k)]
        rng.shuffle(al)
    out = al[0]
    for a in al[1:]:
        out += ("|" if rng.random() < 0.5 else "/") + a
    return out


def cell_of_code(rng, code, num_allele, extras=(0, 3)):
    """the GT and between extras[0] and extras[1] further sub-fields of 1 to 6 characters"""
    n = int(rng.integers(extras[0], extras[1] + 1))
    subs = ["".join(rng.choice(list("0123456789.,"), size=int(rng.integers(1, 7)))) for _ in range(n)]
    return ":".join([gt_of_code(rng, code, num_allele)] + subs)


def fixed_columns(i, num_allele, id_len=None, chrom="1"):
    """CHROM ... FORMAT of variant i; id_len sets the length of the ID and with it the byte phase of the line's cells"""
    vid = "." if id_len == 0 else ("rs%d" % (i + 1)).ljust(id_len or 0, "x")
    alt = "." if num_allele == 1 else ",".join(ALT_POOL[:num_allele - 1])
    return [chrom, str(1000 + 7 * i), vid, "A", alt, str(10 + i % 50), "PASS" if i % 3 else ".", "NS=%d" % (i % 9), "GT:X:Y:Z"]


def make_lines(codes, seed=0, num_allele=None, extras=(0, 3), id_lens=None):
    """one list of cells per row of `codes` ([L][n] values 0 ... 3) and the fixed columns of every line:
    (fixed [L] lists of 9 str, cells [L] lists of n str, num_allele [L])"""
    rng = np.random.default_rng(seed)
    codes = np.asarray(codes)
    L, n = codes.shape
    na = [int(rng.integers(2, 13)) for _ in range(L)] if num_allele is None else [int(x) for x in np.broadcast_to(num_allele, (L,))]
    fixed = [fixed_columns(i, na[i], None if id_lens is None else id_lens[i % len(id_lens)]) for i in range(L)]
    cells = [[cell_of_code(rng, int(codes[i, j]), na[i], extras) for j in range(n)] for i in range(L)]
    return fixed, cells, na


def join_lines(fixed, cells, newline="\n", final_newline=True):
    """the data lines as one str"""
    t = newline.join("\t".join(f + c) for f, c in zip(fixed, cells))
    return t + (newline if final_newline else "")


def vcf_text(fixed, cells, sample_ids=None, newline="\n", final_newline=True):
    """a whole file: header, #CHROM line, data lines"""
    n = len(cells[0])
    ids = ["S%03d" % j for j in range(n)] if sample_ids is None else list(sample_ids)
    head = HEADER.replace("\n", newline) + "\t".join("#CHROM POS ID REF ALT QUAL FILTER INFO FORMAT".split() + ids) + newline
    return head + join_lines(fixed, cells, newline, final_newline)


def python_index(data):
    """(col_begin [L][10], line_end [L]) of data lines (bytes) by split alone: what snpgpu_vcf_index has to return"""
    cols, ends, pos = [], [], 0
    for raw in data.split(b"\n"):
        if pos >= len(data):
            break
        line = raw[:-1] if raw.endswith(b"\r") else raw
        parts = line.split(b"\t")
        off, p = [], pos
        for c in parts[:10]:
            off.append(p)
            p += len(c) + 1
        cols.append(off)
        ends.append(pos + len(line))
        pos += len(raw) + 1
    return np.array(cols, np.int64).reshape(-1, 10), np.array(ends, np.int64)
