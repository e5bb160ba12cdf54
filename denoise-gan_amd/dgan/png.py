"""A PNG encoder for 8-bit RGB frames without a codec library: the numpy definition of the file and
the device op (csrc/png_enc.hip) equal to it byte for byte.  The file is this module's own: any PNG
reader decodes it to the input, but it is not the file zlib or Pillow would write.

    container  signature, IHDR (8 bits, colour type 2, no interlace), one IDAT chunk per deflate
               block, a last IDAT chunk of 9 bytes (the final empty stored block and the Adler-32),
               IEND; no ancillary chunks.  A chunk's CRC-32 depends on its own block only.
    filter     per row the five PNG filters with bpp 3, the row above as the raw prior (zeros above
               row 0); the winner has the smallest sum of min(v, 256 - v) over its bytes, the lower
               type on a tie (libpng's heuristic).  The filtered stream is h rows of 3 w + 1 bytes.
    deflate    one zlib stream (header 78 01).  The stream is cut into spans of SPAN = 32768 bytes
               (the last may be shorter), each one deflate block that reads nothing outside it.
      tokens   every maximal run of one byte value inside a span, of length L: the first byte a
               literal; of the R = L - 1 others, R // 258 matches of length 258 at distance 1, then
               the remainder r as one match if r >= 3, else r literals; then the end-of-block symbol
      codes    dynamic Huffman codes from the block's own counts, literal/length codes of at most
               15 bits, the code-length code of at most 7; one distance code of one bit when the
               block has a match, else one of zero bits.  Lengths (`code_lengths`): the used symbols
               sorted by (count, symbol); Huffman's algorithm with two queues, leaves and merged
               nodes, which takes the leaf when the two heads weigh the same; the leaves' depths
               counted per length, depths past the limit counted at the limit; while the Kraft sum
               exceeds 1, one code leaves the limit and the longest shorter length gives one code to
               the length below it, which gains two (miniz's repair); then the lengths go to the
               sorted symbols, the longest first.  One used symbol gets one bit.
      header   the lengths of the literal/length codes up to the last used one and the distance
               code's as one sequence; a run of zeros as 18s of up to 138 while 11 or more are
               left, then one 17 if 3 or more are, else single zeros; a run of another length as the
               length once, 16s of up to 6 while 3 or more are left, then the length itself
      joining  a dynamic block is followed by an empty stored block (three zero bits, zeros up to the
               byte, 00 00 ff ff), so every block starts on a byte.  A span is stored (00, LEN, NLEN,
               the bytes) whenever that is not longer than the dynamic block with its 4 + bytes.
               No block carries the final bit; the last chunk's empty stored block does.

`png_filter_ref`, `deflate_ref` and `png_encode_ref` are pure numpy and import neither torch nor the
library.  `png_encode` is the device op.
"""
import numpy as np

SPAN = 32768
SIGNATURE = b"\x89PNG\r\n\x1a\n"
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_CRC_TABLE = np.zeros(256, np.uint32)
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = (_c >> 1) ^ 0xEDB88320 if _c & 1 else _c >> 1
    _CRC_TABLE[_i] = _c
_CRC_LIST = _CRC_TABLE.tolist()


def crc32(data):
    c = 0xFFFFFFFF
    for b in bytes(data):
        c = _CRC_LIST[(c ^ b) & 255] ^ (c >> 8)
    return c ^ 0xFFFFFFFF


def adler32(data):
    d = np.frombuffer(bytes(data), np.uint8).astype(np.int64)
    a = (1 + int(d.sum())) % 65521
    b = (d.size + int((d * np.arange(d.size, 0, -1)).sum())) % 65521
    return (b << 16) | a


def _chunk(kind, payload):
    return len(payload).to_bytes(4, "big") + kind + payload + crc32(kind + payload).to_bytes(4, "big")


def _check_image(a, what):
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[-1] != 3:
        raise ValueError(f"{what}: expected uint8 [h,w,3], got {a.dtype} {a.shape}")
    if min(a.shape[:2]) < 1:
        raise ValueError(f"{what}: empty image: {a.shape}")
    if max(a.shape[:2]) > 65535:
        raise ValueError(f"{what}: at most 65535 rows and columns, got {a.shape[0]}x{a.shape[1]}")
    return a


def png_filter_ref(img_u8):
    """One uint8 [h,w,3] image -> the filtered stream, `bytes` of h (3 w + 1) (module docstring)."""
    a = _check_image(img_u8, "png_filter_ref")
    h, w = a.shape[:2]
    x = a.reshape(h, 3 * w).astype(np.int64)
    left = np.pad(x, ((0, 0), (3, 0)))[:, :3 * w]
    up = np.pad(x, ((1, 0), (0, 0)))[:h]
    ul = np.pad(up, ((0, 0), (3, 0)))[:, :3 * w]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = np.stack([x, x - left, x - up, x - (left + up) // 2, x - paeth]) & 255
    best = np.argmin(np.minimum(cand, 256 - cand).sum(axis=2), axis=0)   # the first minimum: the lower type
    out = np.empty((h, 3 * w + 1), np.uint8)
    out[:, 0] = best
    out[:, 1:] = cand[best, np.arange(h)]
    return out.tobytes()


def code_lengths(counts, limit):
    """The code lengths of the symbols with counts[s] > 0, at most `limit` bits (module docstring:
    codes) -> a list as long as counts, 0 for an unused symbol."""
    used = sorted((s for s in range(len(counts)) if counts[s] > 0), key=lambda s: (counts[s], s))
    n, lens = len(used), [0] * len(counts)
    if n == 1:
        lens[used[0]] = 1
    if n < 2:
        return lens
    leaf = [int(counts[s]) for s in used]
    node, leaf_parent, node_parent, li, ni = [], [0] * n, [0] * (n - 1), 0, 0
    for k in range(n - 1):
        weight = 0
        for _ in range(2):
            if li < n and (ni >= k or leaf[li] <= node[ni]):
                weight, leaf_parent[li], li = weight + leaf[li], k, li + 1
            else:
                weight, node_parent[ni], ni = weight + node[ni], k, ni + 1
        node.append(weight)
    depth = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        depth[k] = depth[node_parent[k]] + 1
    per = [0] * (limit + 1)
    for i in range(n):
        per[min(depth[leaf_parent[i]] + 1, limit)] += 1
    kraft = sum(per[b] << (limit - b) for b in range(1, limit + 1))
    while kraft > 1 << limit:
        per[limit] -= 1
        b = limit - 1
        while not per[b]:
            b -= 1
        per[b], per[b + 1], kraft = per[b] - 1, per[b + 1] + 2, kraft - 1
    i = 0
    for b in range(limit, 0, -1):
        for _ in range(per[b]):
            lens[used[i]], i = b, i + 1
    return lens


def canonical_codes(lens):
    """RFC 1951's codes of the lengths, every code with its first bit lowest (as it is written)."""
    limit = max(max(lens), 1)
    per = [0] * (limit + 2)
    for b in lens:
        per[b] += b > 0
    nxt, code = [0] * (limit + 2), 0
    for b in range(1, limit + 1):
        code = (code + per[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lens)
    for s, b in enumerate(lens):
        if b:
            out[s] = int(format(nxt[b], f"0{b}b")[::-1], 2)
            nxt[b] += 1
    return out


def _tokens(d):
    """A span (uint8 array) -> per byte the literal/length symbol (-1: inside a match), the count of
    extra bits and their value."""
    n = d.size
    i = np.arange(n)
    first = np.ones(n, bool)
    first[1:] = d[1:] != d[:-1]
    start = np.maximum.accumulate(np.where(first, i, 0))
    end = np.append(i[first][1:], n)[np.cumsum(first) - 1]   # the next run's start
    R, q = end - start - 1, i - start - 1
    full = (R // 258) * 258
    in_full = (q >= 0) & (q < full)
    r = R - full
    length = np.where(in_full, np.where(q % 258 == 0, 258, 0), np.where(r >= 3, np.where(q == full, r, 0), 1))
    length[q < 0] = 1   # 1: a literal, 0: nothing, >= 3: a match
    l3 = np.maximum(length - 3, 0)
    e = np.maximum(np.floor(np.log2(np.maximum(l3, 1))).astype(np.int64) - 2, 0)
    sym = np.where(length == 258, 285, np.where(l3 < 8, 257 + l3, 261 + 4 * e + ((l3 >> e) & 3)))
    e[(length == 258) | (length < 3)] = 0
    sym = np.where(length == 1, d, np.where(length == 0, -1, sym))
    return sym, e, l3 & ((1 << e) - 1)


def _header_items(seq):
    """The code lengths `seq` -> [(code-length symbol, extra bits, their value)] (module docstring: header)."""
    items, i = [], 0
    while i < len(seq):
        j = i
        while j < len(seq) and seq[j] == seq[i]:
            j += 1
        v, left = seq[i], j - i
        if v == 0:
            while left >= 11:
                items.append((18, 7, min(left, 138) - 11))
                left -= min(left, 138)
            if left >= 3:
                items.append((17, 3, left - 3))
                left = 0
        else:
            items.append((v, 0, 0))
            left -= 1
            while left >= 3:
                items.append((16, 2, min(left, 6) - 3))
                left -= min(left, 6)
        items += [(v, 0, 0)] * left
        i = j
    return items


def _pack_bits(val, nb):
    """Values `val` of `nb` bits each (arrays), first bit lowest, one after the other -> uint8 bits."""
    val, nb = np.asarray(val, np.int64), np.asarray(nb, np.int64)
    owner = np.repeat(np.arange(nb.size), nb)
    j = np.arange(owner.size) - np.repeat(np.cumsum(nb) - nb, nb)
    return ((val[owner] >> j) & 1).astype(np.uint8)


def _block(d):
    """One span -> its bytes in the stream: the dynamic block and the empty stored block, or the span stored."""
    sym, eb, ev = _tokens(d)
    lit = sym >= 0
    counts = np.bincount(np.append(sym[lit], 256), minlength=286)
    lens = code_lengths(counts.tolist(), 15)
    codes = canonical_codes(lens)
    matches = bool((sym > 256).any())
    nlit = max(s for s in range(286) if lens[s]) + 1
    items = _header_items(lens[:nlit] + [1 if matches else 0])
    cl_lens = code_lengths(np.bincount([it[0] for it in items], minlength=19).tolist(), 7)
    cl_codes = canonical_codes(cl_lens)
    ncl = max(k for k in range(19) if cl_lens[_CL_ORDER[k]]) + 1
    ncl = max(ncl, 4)
    # BFINAL 0, BTYPE 2, HLIT, HDIST 0, HCLEN, the code-length code's lengths, the coded lengths
    val = [0, 2, nlit - 257, 0, ncl - 4] + [cl_lens[_CL_ORDER[k]] for k in range(ncl)]
    nb = [1, 2, 5, 5, 4] + [3] * ncl
    for s, b, v in items:
        val.append(cl_codes[s] | (v << cl_lens[s]))
        nb.append(cl_lens[s] + b)
    L, C = np.array(lens, np.int64), np.array(codes, np.int64)
    s = sym[lit]
    tok_nb = L[s] + eb[lit] + (s > 256)            # a match: its extra bits, then the distance code 0
    tok_val = C[s] | (ev[lit] << L[s])
    val = np.concatenate([val, tok_val, [codes[256]]])
    nb = np.concatenate([nb, tok_nb, [lens[256]]])
    bits = int(nb.sum())
    dynamic = (bits + 3 + 7) // 8 + 4
    if dynamic >= 5 + d.size:
        return bytes([0]) + d.size.to_bytes(2, "little") + (d.size ^ 0xFFFF).to_bytes(2, "little") + d.tobytes()
    stream = np.zeros((dynamic - 4) * 8, np.uint8)
    stream[:bits] = _pack_bits(val, nb)
    return np.packbits(stream, bitorder="little").tobytes() + b"\x00\x00\xff\xff"


def _deflate_parts(data):
    """-> the stream as the payloads of its chunks: one per span (the first with the zlib header), the tail."""
    data = bytes(data)
    d = np.frombuffer(data, np.uint8)
    parts = [_block(d[at:at + SPAN]) for at in range(0, d.size, SPAN)]
    tail = b"\x01\x00\x00\xff\xff" + adler32(data).to_bytes(4, "big")
    if parts:
        return [b"\x78\x01" + parts[0]] + parts[1:] + [tail]
    return [b"\x78\x01" + tail]


def deflate_ref(data):
    """`bytes` -> their zlib stream as this module writes it (module docstring: deflate)."""
    return b"".join(_deflate_parts(data))


def png_header(h, w):
    """Signature and IHDR of an h x w 8-bit RGB file: 33 bytes."""
    if not (1 <= int(h) <= 65535 and 1 <= int(w) <= 65535):
        raise ValueError(f"png_header: at most 65535 rows and columns, got {h}x{w}")
    return SIGNATURE + _chunk(b"IHDR", int(w).to_bytes(4, "big") + int(h).to_bytes(4, "big") + bytes([8, 2, 0, 0, 0]))


def png_encode_ref(img_u8):
    """The encoder's definition on the host: one uint8 [h,w,3] image -> the bytes of its PNG file."""
    a = _check_image(img_u8, "png_encode_ref")
    parts = _deflate_parts(png_filter_ref(a))
    return png_header(a.shape[0], a.shape[1]) + b"".join(_chunk(b"IDAT", p) for p in parts) + _chunk(b"IEND", b"")


# ---------------------------------------------------------------------------
# device code below: torch and the library are imported on use
# ---------------------------------------------------------------------------
class _Plan:
    """The buffers of png_encode at one (n, h, w, device): workspace, files, file lengths."""

    def __init__(self, n, h, w, device):
        import torch
        from . import ops
        ws, stride = ops.png_encode_bytes(n, h, w)
        self.ws = torch.empty(ws, dtype=torch.uint8, device=device)
        self.out = torch.empty((n, stride), dtype=torch.uint8, device=device)
        self.sizes = torch.empty(n, dtype=torch.int32, device=device)


MAX_PLANS = 8   # plans kept, least recently used first out (metrics._lru)
_plans = {}


def clear_plans():
    """Drop every kept plan (their device buffers are freed with them)."""
    _plans.clear()


def _files(out, sizes, least, what):
    """out[i, :sizes[i]] of the device -> a list of `bytes` through one pinned buffer."""
    import torch
    sizes = sizes.cpu().tolist()
    if min(sizes) < least or max(sizes) > out.shape[1]:
        raise RuntimeError(f"{what}: the device reports lengths {sizes}")
    host = torch.empty(sum(sizes), dtype=torch.uint8, pin_memory=True)
    at = 0
    for i, size in enumerate(sizes):
        host[at:at + size].copy_(out[i, :size], non_blocking=True)
        at += size
    torch.cuda.current_stream().synchronize()
    data, files, at = host.numpy().tobytes(), [], 0
    for size in sizes:
        files.append(data[at:at + size])
        at += size
    return files


def png_encode(x):
    """A dense uint8 NHWC device tensor [n,h,w,3] -> a list of n `bytes`, every image's PNG file, equal
    to `png_encode_ref` byte for byte; [] for n = 0.  Filtering, run-length deflate, check sums and
    packing run on the device (csrc/png_enc.hip); what crosses to the host is n file lengths and the
    files.  The call waits for the lengths, so it cannot be captured in a graph; its buffers are
    kept per shape in an LRU of plans."""
    import torch
    from . import ops
    from .metrics import _lru
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise ValueError(f"png_encode: expected a uint8 tensor, got {getattr(x, 'dtype', type(x))}")
    if x.dim() != 4 or x.shape[3] != 3 or not x.is_contiguous() or not x.is_cuda:
        raise ValueError(f"png_encode: expected a dense [n,h,w,3] device tensor, got shape {tuple(x.shape)} on "
                         f"{x.device}")
    n, h, w, _ = x.shape
    if min(h, w) < 1:
        raise ValueError(f"png_encode: empty image: {tuple(x.shape)}")
    header = png_header(h, w)
    if n == 0:
        return []
    p = _lru(_plans, (n, h, w, x.device), lambda: _Plan(n, h, w, x.device), MAX_PLANS)
    ops.png_encode(x, header, p.ws, p.out, p.sizes)
    return _files(p.out, p.sizes, len(header) + 33, "png_encode")
