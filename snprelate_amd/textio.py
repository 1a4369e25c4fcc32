"""What the readers of text formats share on the host (vcf.py, ped.py, gen.py): a file read in chunks of whole lines through two
buffers, the lines of a chunk, the restatement of the reference's ``CReadLine::GetCell`` and the leading columns of every line
read with it.  Nothing here needs a device; a reader adds its format's columns and its calls into libsnpgpu.
"""
import gzip
import os

import numpy as np

HEAD = 1024            # bytes of a line looked at for its leading columns before the whole line is taken


class VcfFormatError(ValueError):
    """an error of the reference's parser: .message is its text, .column / .cell what COREARRAY_TRY_END appends"""

    def __init__(self, message, column=0, cell=b""):
        ValueError.__init__(self, message)
        self.message, self.column, self.cell = message, int(column), cell


def open_binary(fn):
    return gzip.open(fn, "rb") if str(fn).lower().endswith(".gz") else open(fn, "rb")


def stage_bytes():
    return max(1, int(os.environ.get("SNPGPU_TEXT_STAGE_BYTES", 256 << 20)))


# ---- a file in chunks of whole lines ---------------------------------------------------------------------------------------------
def chunks(f, buffers, index, path, env_name):
    """The binary file object `f` read front to back through `buffers`, two uint8 arrays of one size, in turn.  index(buf, n,
    final) finds the whole lines of buf[:n] -- `final`: the file ends with them -- and returns a tuple that ends with the bytes
    they take; the chunk is yielded as (buf, n, final) + the rest of that tuple.  The cut line behind them moves to the head of
    the other buffer, so a yielded buffer is as it was until the chunk after the next one is asked for.  A chunk that is not the
    last and holds no whole line is an error that names the file `path` and `env_name`, the variable that sizes the buffers."""
    size = min(len(b) for b in buffers)
    turn, left = 0, 0                                     # `left` bytes of a cut line stand at the head of buffers[turn]
    while True:
        buf = buffers[turn]
        n = left
        while n < size:
            got = f.readinto(memoryview(buf)[n:size])
            if not got:
                break
            n += got
        final = n < size
        if n == 0:
            break
        *found, used = index(buf, n, final)
        if used == 0 and not final:
            raise ValueError("'%s': a line longer than the %d bytes of a chunk (%s)" % (path, size, env_name))
        yield (buf, n, final, *found)
        left = n - used
        if left:
            buffers[1 - turn][:left] = buf[used:n]
        turn = 1 - turn
        if final:
            break


def split_lines(buf, n, final, strip_cr):
    """the whole lines of buf[:n]: (begin, end) arrays without the '\\n' -- with strip_cr without a '\\r' in front of it too -- and
    the bytes consumed"""
    nl = np.flatnonzero(buf[:n] == 10)
    begin = np.concatenate(([0], nl + 1)).astype(np.int64)
    end = nl.astype(np.int64)
    used = int(nl[-1]) + 1 if len(nl) else 0
    if final and used < n:
        end = np.concatenate((end, [n]))
        used = n
    else:
        begin = begin[:len(end)]
    if strip_cr:
        end = end - ((end > begin) & (buf[np.maximum(end - 1, 0)] == 13))
    return begin, end, used


# ---- a line on the host ----------------------------------------------------------------------------------------------------------
class Cells:
    """CReadLine::GetCell over one line (src/ConvToGDS.cpp:123-179): the column count, the end-of-line checks and the quotes it
    strips.  Split by tabs as gnrParseVCF4 sets it, or with `space` by tab and space as gnrParsePED does (SplitBySpaceTab): one
    tab is one separator, a run of spaces is one separator, and spaces behind the last column are skipped.  `cell` is what the
    reference's `cell` variable holds when an error is formatted."""

    def __init__(self, line, pos=0, column=0, cell=b"", space=False):
        self.s, self.p, self.column, self.cell, self.space = line, pos, column, cell, space

    def get(self, last):
        s, b = self.s, self.p
        e = s.find(b"\t", b)
        if self.space:
            e2 = s.find(b" ", b, e if e >= 0 else len(s))
            e = e2 if e2 >= 0 else e
        at_end = e < 0
        if at_end:
            e = len(s)
        self.column += 1
        if b == e and at_end:
            raise VcfFormatError("fewer columns than what expected.", self.column, self.cell)
        p = e
        if last:
            if self.space:
                while p < len(s) and s[p] == 0x20:
                    p += 1
            if p < len(s):
                raise VcfFormatError("more columns than what expected.", self.column, self.cell)
            self.p = p
        elif at_end:
            self.p = e
        elif s[e] == 0x09 or not self.space:
            self.p = e + 1
        else:
            while p < len(s) and s[p] == 0x20:
                p += 1
            self.p = p
        if e > b + 1 and ((s[b] == 0x22 and s[e - 1] == 0x22) or (s[b] == 0x27 and s[e - 1] == 0x27)):
            b, e = b + 1, e - 1
        self.cell = s[b:e]
        return self.cell


def c_string(line):
    z = line.find(b"\0")
    return line if z < 0 else line[:z]


def last_cell(line):
    """the last cell of a line that was read without an error: what the reference's `cell` variable still holds when the first
    cell of the next line fails"""
    s = c_string(line).rstrip(b" ")
    c = s[max(s.rfind(b"\t"), s.rfind(b" ")) + 1:]
    return c[1:-1] if len(c) > 1 and c[0] == c[-1] and c[0] in b"\"'" else c


def read_head(buf, b, e, host_head):
    """host_head -- a format's (leading cells, offset of the cell behind them) of a line given as bytes -- of the line buf[b:e]:
    from the line's first HEAD bytes when they hold the leading cells, else from the whole line"""
    head = bytes(buf[b:min(e, b + HEAD)])
    if e - b > HEAD or b"\0" in head:
        if b"\0" not in head:
            try:
                cells, p = host_head(head)
                if p < len(head):
                    return cells, p
            except VcfFormatError:
                pass
        head = c_string(bytes(buf[b:e]))
    return host_head(head)


def leading_columns(buf, begin, end, host_head, tail):
    """read_head of the lines buf[begin[i]:end[i]], up to the first one that fails: (cell_begin int64, the leading cells per
    line, that line's VcfFormatError or None).  cell_begin is the offset in buf of the cell behind the leading ones.  An error in
    column 1 has read no cell of its line: its `cell` is the last one of the line before, `tail` for the first line."""
    cell_begin, heads = np.empty(len(begin), np.int64), []
    for i in range(len(begin)):
        b, e = int(begin[i]), int(end[i])
        try:
            cells, p = read_head(buf, b, e, host_head)
        except VcfFormatError as err:
            if err.column == 1:
                err.cell = last_cell(bytes(buf[int(begin[i - 1]):int(end[i - 1])])) if i else tail
            return cell_begin[:i], heads, err
        cell_begin[i] = b + p
        heads.append(cells)
    return cell_begin, heads, None
