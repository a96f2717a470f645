"""Model check of the BF tie sort used by the env kernels (csrc/vmp_np_sort.h
wave_aquicksort / aquicksort_lds): numpy's scalar introsort (aquicksort_ +
aheapsort_, npysort) restated serially, against the two transformations the
kernels make — (1) only partitions intersecting the needed position range are
sorted, (2) each Hoare partition is computed from the left/right stop lists
(A, B, K = #{A[k] < B[k]}, final stop min(A[K], B[K-1])) and small partitions
by a stable rank sort. Heavy ties, random ranges and forced depth-limit
heapsorts; positions lo..hi must equal the full serial sort's exactly.

The model also reports whether the depth limit sent a partition to heapsort
(info["heapsort"]), and adversary_keys builds, with McIlroy's adversary ("A
Killer Adversary for Quicksort", 1999) run against this model, a key order
that drives the real depth limit: tests/test_gpu_prims.py feeds those keys to
the device's sorts."""
import numpy as np

from oracle import oracle as O
from tests import prims_cases as C

def fless(a,b): return a<b
def heapsort(v,t,off,n):
    a=lambda i: t[off+i-1]
    def seta(i,x): t[off+i-1]=x
    l=n>>1
    while l>0:
        tmp=a(l); i=l; j=l<<1
        while j<=n:
            if j<n and fless(v[a(j)],v[a(j+1)]): j+=1
            if fless(v[tmp],v[a(j)]): seta(i,a(j)); i=j; j+=j
            else: break
        seta(i,tmp); l-=1
    while n>1:
        tmp=a(n); seta(n,a(1)); n-=1; i=1; j=2
        while j<=n:
            if j<n and fless(v[a(j)],v[a(j+1)]): j+=1
            if fless(v[tmp],v[a(j)]): seta(i,a(j)); i=j; j+=j
            else: break
        seta(i,tmp)
def serial(v,num,lo,hi,par=False,depthcap=None,info=None):
    t=list(range(num)); stack=[]; pl,pr=0,num-1
    cd=0;u=num
    while True:
        u>>=1
        if not u: break
        cd+=1
    cd*=2
    if depthcap is not None: cd=depthcap
    while True:
        skip=False
        if pr<lo or pl>hi: skip=True
        elif cd<0:
            heapsort(v,t,pl,pr-pl+1); skip=True
            if info is not None: info["heapsort"]=info.get("heapsort",0)+1
        if not skip:
            while pr-pl>15:
                pm=pl+((pr-pl)>>1)
                if fless(v[t[pm]],v[t[pl]]): t[pm],t[pl]=t[pl],t[pm]
                if fless(v[t[pr]],v[t[pm]]): t[pr],t[pm]=t[pm],t[pr]
                if fless(v[t[pm]],v[t[pl]]): t[pm],t[pl]=t[pl],t[pm]
                vp=v[t[pm]]; pj=pr-1
                t[pm],t[pj]=t[pj],t[pm]
                if not par:
                    pi=pl
                    while True:
                        pi+=1
                        while fless(v[t[pi]],vp): pi+=1
                        pj-=1
                        while fless(vp,v[t[pj]]): pj-=1
                        if pi>=pj: break
                        t[pi],t[pj]=t[pj],t[pi]
                else:
                    B=[q for q in range(pr-2,pl-1,-1) if not fless(vp,v[t[q]])]
                    A=[q for q in range(pl+1,pr) if not fless(v[t[q]],vp)]
                    K=sum(1 for k in range(min(len(A),len(B))) if A[k]<B[k])
                    for k in range(K): t[A[k]],t[B[k]]=t[B[k]],t[A[k]]
                    pi=A[K]
                    if K>0 and B[K-1]<pi: pi=B[K-1]
                pk=pr-1; t[pi],t[pk]=t[pk],t[pi]
                if pi-pl<pr-pi: stack.append((pi+1,pr,cd-1)); pr=pi-1
                else: stack.append((pl,pi-1,cd-1)); pl=pi+1
                cd-=1
                if pr<lo or pl>hi: skip=True; break
            if not skip:
                if par:
                    seg=t[pl:pr+1]; n=len(seg)
                    out=[None]*n
                    for i in range(n):
                        r=sum(1 for j in range(n) if fless(v[seg[j]],v[seg[i]]) or (j<i and not fless(v[seg[i]],v[seg[j]])))
                        out[r]=seg[i]
                    t[pl:pr+1]=out
                else:
                    for pi in range(pl+1,pr+1):
                        vi=t[pi]; vv=v[vi]; pj=pi; pk=pi-1
                        while pj>pl and fless(vv,v[t[pk]]): t[pj]=t[pk]; pj-=1; pk-=1
                        t[pj]=vi
        if not stack: break
        pl,pr,cd=stack.pop()
    return t


def test_parallel_partition_and_range_sort_equal_serial_introsort():
    rng = np.random.default_rng(1)
    for it in range(600):
        n = int(rng.integers(1, 300))
        nv = int(rng.integers(1, 30))
        v = list(rng.integers(0, nv, n).astype(np.float32))
        lo = int(rng.integers(0, n))
        hi = int(rng.integers(lo, n))
        dc = None if it % 5 else int(rng.integers(-1, 3))
        full = serial(v, n, 0, n - 1, depthcap=dc)
        assert sorted(full) == list(range(n))
        assert all(v[full[i]] <= v[full[i + 1]] for i in range(n - 1))
        for par in (False, True):
            r = serial(v, n, lo, hi, par, depthcap=dc)
            assert r[lo:hi + 1] == full[lo:hi + 1], (n, nv, lo, hi, par)


def select_walk(v,num,lo,hi,carry=True):
    """The order of work of wave_aqselect_top without its early exit: after a
    partition the upper part goes on and the lower part waits. numpy tests
    the depth limit only on a part it pops (the larger one); carry=True
    carries that bit with every part, carry=False is the walk that tested
    every popped lower part and no upper part."""
    t=list(range(num)); stack=[]; pl,pr=0,num-1
    cd=0;u=num
    while True:
        u>>=1
        if not u: break
        cd+=1
    cd*=2
    cont=False
    while True:
        skip=pr<lo or pl>hi
        if not skip and cd<0 and not cont:
            heapsort(v,t,pl,pr-pl+1); skip=True
        if not skip:
            again=False
            while pr-pl>15:
                pm=pl+((pr-pl)>>1)
                if fless(v[t[pm]],v[t[pl]]): t[pm],t[pl]=t[pl],t[pm]
                if fless(v[t[pr]],v[t[pm]]): t[pr],t[pm]=t[pm],t[pr]
                if fless(v[t[pm]],v[t[pl]]): t[pm],t[pl]=t[pl],t[pm]
                vp=v[t[pm]]; pj=pr-1
                t[pm],t[pj]=t[pj],t[pm]
                pi=pl
                while True:
                    pi+=1
                    while fless(v[t[pi]],vp): pi+=1
                    pj-=1
                    while fless(vp,v[t[pj]]): pj-=1
                    if pi>=pj: break
                    t[pi],t[pj]=t[pj],t[pi]
                pk=pr-1; t[pi],t[pk]=t[pk],t[pi]
                lower_small=pi-pl<pr-pi
                cd-=1
                stack.append((pl,pi-1,cd,lower_small if carry else False))
                pl=pi+1
                cont=(not lower_small) if carry else True
                if pr<lo or pl>hi: skip=True; break
                if not cont and cd<0: again=True; break
            if again: continue
            if not skip:
                for pi in range(pl+1,pr+1):
                    vi=t[pi]; vv=v[vi]; pj=pi; pk=pi-1
                    while pj>pl and fless(vv,v[t[pk]]): t[pj]=t[pk]; pj-=1; pk-=1
                    t[pj]=vi
        if not stack: break
        pl,pr,cd,cont=stack.pop()
    return t


class _Gas:
    """Key i of McIlroy's adversary: undecided ("gas") until a comparison
    forces a value. Two gas keys compared: the one that is not the current
    pivot candidate freezes at the next free value; gas is above every frozen
    value. Every answer stays consistent with the values left at the end."""
    def __init__(self, adv, i): self.adv, self.i = adv, i
    def __lt__(self, other): return self.adv.less(self.i, other.i)


class _Adversary:
    def __init__(self, n):
        self.gas = n
        self.val = [n] * n
        self.nsolid = 0
        self.candidate = 0
    def __getitem__(self, i): return _Gas(self, i)
    def less(self, x, y):
        val, gas = self.val, self.gas
        if val[x] == gas and val[y] == gas:
            z = x if x == self.candidate else y
            val[z] = self.nsolid
            self.nsolid += 1
        if val[x] == gas: self.candidate = x
        elif val[y] == gas: self.candidate = y
        return val[x] < val[y]


def adversary_keys(n):
    """float32 keys [n] (integers <= n, exact) on which the introsort's
    median-of-three partitions peel off a few elements each."""
    adv = _Adversary(n)
    serial(adv, n, 0, n - 1)
    return np.array(adv.val, np.float32)


def test_adversary_keys_drive_the_depth_limit():
    """On the adversary's keys the model runs heapsort at every n >= 129 of
    the device tests, and the model's order is the oracle's."""
    for n in C.SORT_N:
        if n < 129:
            continue
        keys = adversary_keys(n)
        info = {}
        full = serial(list(keys), n, 0, n - 1, info=info)
        assert info.get("heapsort", 0) > 0, n
        out = np.zeros(n, np.int64)
        O.lib().oracle_argsort_f32(O._p(keys), n, O._p(out))
        assert full == out.tolist(), n


def test_select_walk_meets_the_depth_limit_where_numpy_does():
    """Organ pipe and adversary keys reach the depth limit. The walk of
    wave_aqselect_top equals the full sort on every range only if each part
    carries whether numpy pops it (depth test) or goes on with it (none)."""
    wrong_without = 0
    for n in (129, 200, 1000):
        i = np.arange(n)
        for k, keys in enumerate((adversary_keys(n), (np.minimum(i, n - 1 - i) / 8).astype(np.float32))):
            v = list(keys)
            info = {}
            full = serial(v, n, 0, n - 1, info=info)
            assert info.get("heapsort", 0) > 0 or (k == 1 and n < 1000), n  # the pipe: at 1000
            rng = np.random.default_rng(n)
            ranges = [(0, n - 1), (n // 2, n // 2)] + \
                [tuple(sorted(rng.integers(0, n, 2).tolist())) for _ in range(6)]
            for lo, hi in ranges:
                assert select_walk(v, n, lo, hi)[lo:hi + 1] == full[lo:hi + 1], (n, lo, hi)
                wrong_without += select_walk(v, n, lo, hi, carry=False)[lo:hi + 1] != full[lo:hi + 1]
    assert wrong_without > 0
