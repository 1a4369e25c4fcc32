"""numpy restatement of the PLINK .bed layout and of snpgpu_geno_convert (include/snpgpu.h section 1k), bit by bit through
np.unpackbits / np.packbits and the reference's two tables, independent of pack_2bit_rows / unpack_2bit_rows and of
snprelate_amd/bed.py.  Codes are uint8 [L][n] (SNP x sample) throughout; "GDS" codes count A alleles (3 = missing, padding 3),
"BED" codes are PLINK's (1 = missing, padding 0)."""
import numpy as np

import geno_select_ref as R

GDS, BED = 0, 1
BED_TO_GDS = np.array([2, 3, 1, 0], np.uint8)            # src/ConvToGDS.cpp:585
GDS_TO_BED = np.array([3, 2, 0, 1], np.uint8)            # src/SNPRelate.cpp:801
PAD = {GDS: 3, BED: 0}


def pack_rows(m, pad):
    """codes [rows][cols] -> bytes [rows][ceil(cols / 4)], code j at bits 2 (j % 4) of byte j // 4, unused codes `pad`"""
    rows, cols = m.shape
    rb = (cols + 3) // 4
    b = np.full((rows, 8 * rb), 0, np.uint8)
    b[:, 0::2], b[:, 1::2] = pad & 1, pad >> 1
    b[:, 0:2 * cols:2] = m & 1
    b[:, 1:2 * cols:2] = m >> 1
    return np.packbits(b, axis=1, bitorder="little")


def unpack_rows(data, rows, cols):
    """bytes [rows][ceil(cols / 4)] -> codes [rows][cols]"""
    bits = np.unpackbits(np.ascontiguousarray(data, dtype=np.uint8).reshape(rows, -1), axis=1, bitorder="little")
    return (bits[:, 0:2 * cols:2] | (bits[:, 1:2 * cols:2] << 1)).astype(np.uint8)


def recode(g, src_code, dst_code):
    if src_code == dst_code:
        return g
    return (BED_TO_GDS if src_code == BED else GDS_TO_BED)[g]


def bed_body(g_gds, mode):
    """GDS codes [L][n] -> the bytes after the header of a .bed file of `mode` (1: SNP rows, 0: sample rows)"""
    b = GDS_TO_BED[g_gds]
    return pack_rows(b if mode == 1 else b.T, 0)


def bed_file(g_gds, mode):
    return bytes([0x6C, 0x1B, mode]) + bed_body(g_gds, mode).tobytes()


def bed_codes(data, mode, n_snp, n_samp):
    """the bytes of a whole .bed file -> GDS codes [L][n]"""
    d = np.frombuffer(bytes(data), np.uint8)
    assert d[0] == 0x6C and d[1] == 0x1B and d[2] == mode
    rows, cols = (n_snp, n_samp) if mode == 1 else (n_samp, n_snp)
    m = BED_TO_GDS[unpack_rows(d[3:], rows, cols)]
    return m if mode == 1 else np.ascontiguousarray(m.T)


def source_codes(data, kw):
    """the codes [snp][sample] a stream description (geno_select_ref.make_stream) holds, whatever they mean"""
    n_rows, n_cols = kw["n_rows"], kw["n_cols"]
    bits = np.unpackbits(np.ascontiguousarray(data, dtype=np.uint8), bitorder="little")
    if kw.get("row_bit") is not None:
        start = kw["bit0"] + np.asarray(kw["row_bit"], np.int64)
    else:
        start = kw["bit0"] + np.arange(n_rows, dtype=np.int64) * kw["row_stride_bits"]
    pos = start[:, None] + 2 * np.arange(n_cols, dtype=np.int64)[None, :]
    codes = bits[pos] | (bits[pos + 1] << 1)
    return codes.T if kw["major"] else codes


def convert_ref(data, kw, src_code, dst_code, dst_major, samp_index=None, snp_index=None, codes=None):
    """what snpgpu_geno_convert writes: uint8 [n_snp_out][ceil(n_samp_out / 4)] for dst_major 0, [n_samp_out][ceil(n_snp_out / 4)]
    for dst_major 1, in dst_code with its padding.  codes: source_codes(data, kw) when the caller has them already"""
    g = source_codes(data, kw) if codes is None else codes
    if snp_index is not None:
        g = g[np.asarray(snp_index, np.int64)]
    if samp_index is not None:
        g = g[:, np.asarray(samp_index, np.int64)]
    g = recode(g, src_code, dst_code)
    return pack_rows(g.T if dst_major else g, PAD[dst_code])


def padding_ok(out, n_cols, dst_code):
    """the unused codes of every row's last byte are dst's padding (all ones for GDS, zero for BED)"""
    r = n_cols % 4
    if not r:
        return True
    tail = out[:, -1] >> (2 * r)
    return bool((tail == ((0xFF >> (2 * r)) if dst_code == GDS else 0)).all())


# the lists and shapes of the selection tests serve here as they are
SAMPLES, SNPS, MISSING, LAYOUTS = R.SAMPLES, R.SNPS, R.MISSING, R.LAYOUTS
