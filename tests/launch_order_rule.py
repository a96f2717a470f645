"""The launch order of the heuristic per-step launch ("Launch
order"; csrc/vmp_launch_order.h) restated with lists, for the tests: which env
each workgroup takes, given the launch's parity and the flag bytes it reads."""
import numpy as np

DIV = 4  # tail ranks T = nr / 4, the library's default


def chunks(n):
    return (n + 63) // 64


def ranks(n):
    return n // chunks(n)


def tail(n, div=DIV):
    return 0 if ranks(n) < 8 else ranks(n) // div


def position(n, parity, block):
    """Dispatch position of a workgroup: upward launches walk the envs upwards."""
    return n - 1 - block if parity else block


def _ends(n, parity, div):
    """(late ranks, early ranks), ascending: late are the T dispatched last."""
    nr, t = ranks(n), tail(n, div)
    low, high = list(range(t)), list(range(nr - t, nr))
    return (low, high) if parity else (high, low)


def chunk_map(n, parity, line, div=DIV):
    """rank -> the rank whose env it runs, for one chunk's 64 flag bytes."""
    late, early = _ends(n, parity, div)
    a = [r for r in late if line[r] != 0]
    b = [r for r in early if line[r] == 0]
    m = list(range(ranks(n)))
    for x, y in zip(a, b):
        m[x], m[y] = y, x
    return m


def env_of_block(n, parity, flags, div=DIV):
    """int64 [n]: the env of every workgroup of a mode-2 launch."""
    c_n, nr = chunks(n), ranks(n)
    flags = np.asarray(flags).reshape(c_n, 64)
    maps = [chunk_map(n, parity, flags[c], div) for c in range(c_n)]
    out = np.empty(n, np.int64)
    for blk in range(n):
        q = position(n, parity, blk)
        r, c = divmod(q, c_n)
        out[blk] = maps[c][r] * c_n + c if r < nr else q
    return out


def late_busy_expected(n, parity, flags, div=DIV):
    """Busy envs that must stay in late ranks: sum over chunks of max(0, |A| - |B|)."""
    flags = np.asarray(flags).reshape(chunks(n), 64)
    late, early = _ends(n, parity, div)
    return sum(max(0, int((f[late] != 0).sum()) - int((f[early] == 0).sum())) for f in flags)


def late_busy_left(n, parity, flags, env_of_blk, div=DIV):
    """Busy envs that a launch with this map runs in late ranks."""
    c_n = chunks(n)
    flags = np.asarray(flags).reshape(c_n, 64)
    late, _ = _ends(n, parity, div)
    left = 0
    for blk in range(n):
        q = position(n, parity, blk)
        r, c = divmod(q, c_n)
        if r in late:
            e = int(env_of_blk[blk])
            left += int(flags[e % c_n, e // c_n] != 0)
    return left
