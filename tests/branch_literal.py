"""Truth model of vmp_branch (include/vmp.h) on snapshot bytes.

TEST INFRASTRUCTURE ONLY. From the snapshot bytes of src and dst, a map and
seeds, `branch` produces the snapshot bytes dst must have after
vmp_branch(dst, src, map, seeds): every env's three rows copied whole, the
streams of reseeded envs taken from numpy itself.

Snapshot parts (the offsets tests/test_gpu_series.py::_assert_same_snapshot
reports by): descriptor 256 B | hdr N x 256 B | pm N x 2P f64 | VM words
N x 4 pitch(V) B. Header words used here (csrc/vmp_layout.h EnvHdr, u64
index): rng[k] = 4k .. 4k+3 as [state_hi, state_lo, inc_hi, inc_lo],
seqbase[j] = 16 + 2j, 17 + 2j (the state of stream j at the last reset),
timestep 20, total_requests 21, served 22, suspend 23, place 24, dropped 25,
the step hint word `pad` 31."""
import numpy as np

DESC = 256
HDR = 256
W_TIMESTEP, W_TOTAL, W_PAD = 20, 21, 31
M64 = (1 << 64) - 1


def pitch(V):
    """vm_pitch (csrc/vmp_layout.h): u32 words of an env's VM row."""
    b = (V + 63) >> 6
    if V <= 1024:
        q = 1
        while q < b:
            q <<= 1
        b = q
    return b << 7


def parts(n, P, V):
    """Byte offsets (hdr, pm, vmw, end) of a plain n-env snapshot."""
    hdr = DESC
    pm = hdr + HDR * n
    vmw = pm + 16 * P * n
    return hdr, pm, vmw, vmw + 4 * pitch(V) * n


def rows(snap, n, P, V):
    """Views (hdr [n, 256], pm [n, 16P], vmw [n, 4 pitch]) into snapshot bytes."""
    snap = np.asarray(snap, np.uint8)
    h, p, v, end = parts(n, P, V)
    assert snap.size >= end, (snap.size, end)
    return (snap[h:p].reshape(n, HDR), snap[p:v].reshape(n, 16 * P), snap[v:end].reshape(n, 4 * pitch(V)))


def hdr_words(snap, n, P, V):
    """u64 [n, 32] copy of the headers."""
    return rows(snap, n, P, V)[0].copy().view(np.uint64)


def stream_words(seed):
    """The 10 u64 words k_reset writes for reset(seed): rng[0..3] then
    seqbase[0..1], from numpy's own PCG64(seed + k)."""
    w = []
    states = []
    for k in range(4):
        st = np.random.PCG64(int(seed) + k).state["state"]
        s, inc = int(st["state"]), int(st["inc"])
        states.append(s)
        w += [s >> 64, s & M64, inc >> 64, inc & M64]
    for j in range(2):
        w += [states[j] >> 64, states[j] & M64]
    return np.array(w, np.uint64)


def branch(src, dst, n_src, n_dst, P, V, index, seeds=None):
    """Expected dst snapshot bytes. index int [n_dst]: entries outside
    [0, n_src) keep the env. seeds int [n_dst] or None: >= 0 reseeds a copied
    env. The descriptor and anything behind the VM words stay dst's."""
    src, out = np.asarray(src, np.uint8), np.asarray(dst, np.uint8).copy()
    index = np.asarray(index, np.int64)
    assert index.shape == (n_dst,)
    s_rows, d_rows = rows(src.copy(), n_src, P, V), rows(out, n_dst, P, V)
    for i, s in enumerate(index):
        if not 0 <= s < n_src:
            continue
        for sr, dr in zip(s_rows, d_rows):
            dr[i] = sr[s]
        if seeds is not None and int(seeds[i]) >= 0:
            d_rows[0][i, :128] = stream_words(seeds[i])[:16].view(np.uint8)
            d_rows[0][i, 128:160] = stream_words(seeds[i])[16:].view(np.uint8)
    return out
