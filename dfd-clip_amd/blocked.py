"""The fragment-blocked layout of the MLP intermediate `u` (c_fc -> c_proj), restated from csrc/gemm_blocked.hpp for tests
and for anything that must look at `u` by position.

A matrix [M, C] (C % 64 == 0) keeps its footprint, rows rounded up to 16.  Inside a group of 16 rows the order is
[kt = 0 .. C/64)[s = 0..1][er = 0..15][eq = 0..3][16 B]: the 16-byte piece (s, er, eq) of unit (row group, kt) holds
channels 64 kt + 16 eq + 8 s .. + 7 of row er of the group.  Row-group-major, K tile minor."""
import torch

GROUP_ROWS = 16
TILE_CHANNELS = 64


def padded_rows(m):
    return (int(m) + GROUP_ROWS - 1) // GROUP_ROWS * GROUP_ROWS


def piece_offset(row, channel, ld):
    """Element offset (2-byte elements) of `channel` of `row` in a blocked matrix with leading dimension `ld`: the index
    map of gemm_blocked.hpp (dfd_blk_row + K tile * unit + dfd_blk_chunk), in elements instead of bytes."""
    g, er = divmod(int(row), GROUP_ROWS)
    kt, c = divmod(int(channel), TILE_CHANNELS)
    chunk, e = divmod(c, 8)
    s, eq = chunk & 1, chunk >> 1
    return g * GROUP_ROWS * ld + kt * 1024 + s * 512 + er * 32 + eq * 8 + e


def pack(x, fill=0):
    """Row-major [M, C] -> blocked [padded_rows(M), C] (same dtype; the rows beyond M hold `fill`)."""
    m, c = x.shape
    assert c % TILE_CHANNELS == 0, "the blocked layout needs whole 64-channel K tiles"
    mp = padded_rows(m)
    xp = torch.full((mp, c), fill, dtype=x.dtype, device=x.device)
    xp[:m] = x
    v = xp.view(mp // GROUP_ROWS, GROUP_ROWS, c // TILE_CHANNELS, 4, 2, 8)  # [g, er, kt, eq, s, 8]
    return v.permute(0, 2, 4, 1, 3, 5).reshape(mp, c).contiguous()   # [g, kt, s, er, eq, 8]


def unpack(b, m=None):
    """Blocked [rows (a multiple of 16), C] -> row-major [m, C] (m = every row by default)."""
    mp, c = b.shape
    assert mp % GROUP_ROWS == 0 and c % TILE_CHANNELS == 0 and b.is_contiguous()
    v = b.view(mp // GROUP_ROWS, c // TILE_CHANNELS, 2, GROUP_ROWS, 4, 8)  # [g, kt, s, er, eq, 8]
    x = v.permute(0, 3, 1, 4, 2, 5).reshape(mp, c)                   # [g, er, kt, eq, s, 8]
    return x[:mp if m is None else m].contiguous()


def fc_channel_perm(n, device=None):
    """idx [n]: the true output channel that MFMA column c computes once c_fc's weight rows and bias are taken as
    w[idx], b[idx].  Inside every aligned group of 64, column 16 j + 4 eq + e <- channel 16 eq + 4 j + e (its own
    inverse): a lane's accumulator fragments acc[i][0..3] are then 16 consecutive channels of its row."""
    assert n % TILE_CHANNELS == 0
    c = torch.arange(n, device=device)
    return (c & ~60) | ((c & 12) << 2) | ((c & 48) >> 2)


def lane_channels(eq):
    """The true channels (within a 64-channel tile) of lane quarter `eq`'s fragments acc[i][j][e], as [j][e], under
    fc_channel_perm: MFMA column 16 j + 4 eq + e of the tile."""
    perm = fc_channel_perm(TILE_CHANNELS)
    return [[int(perm[16 * j + 4 * eq + e]) for e in range(4)] for j in range(4)]
