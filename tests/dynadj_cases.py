"""K-B (csrc/dynadj.hip) off its six instantiated (V, mid) pairs: inputs for any (V, P, E), the shapes that reach the
run-time form's paths, and the launch arithmetic of the kernel restated in Python (which path a shape takes, how much
LDS each launch asks for).  A plain module: tests/test_dynadj_runtime_gpu.py runs the cases, tests/
test_dynadj_limits_host.py checks — without a GPU — that the table still reaches what it is there for."""
import torch

# (n, Ci, mid, V, P, E): every one takes the run-time instantiation L(0, 0) except <25, 8> at E = 17 and at P = E = 1
RUNTIME_CASES = [
    (3, 8, 8, 18, 5, 15),        # 18 joints (openpose), otherwise the shipped shape
    (2, 16, 12, 25, 5, 15),      # shipped V, mid % 16 != 0
    (2, 8, 6, 25, 5, 15),        # mid % 4 != 0: partial last channel group of the backward's pass 1
    (2, 7, 5, 11, 3, 7),         # everything odd
    (2, 8, 4, 32, 5, 15),        # V = 32: all eight k-steps of the masked sums live, Vp = V
    (2, 8, 16, 8, 2, 4),         # ksplit = 1, forward in two windows
    (2, 16, 32, 11, 3, 5),       # ksplit = 1 at the widest shipped mid
    (2, 8, 17, 11, 3, 7),        # odd mid: forward windows of 8 and 9 channels, ksplit = 1
    (130, 8, 17, 11, 3, 7),      # the same shape past 128 samples: one forward window (fp64 on the GPU, see ref_dev)
    (2, 16, 20, 17, 5, 15),      # shipped V = 17 with an uninstantiated mid
    (2, 64, 36, 25, 5, 15),      # forward 64.8 KB, backward 149 KB: the dynamic-LDS opt-in of L(0, 0), both ways
    (2, 16, 37, 25, 5, 15),      # the largest mid the backward accepts at V = 25 (154.8 KB), odd
    (2, 8, 27, 32, 5, 15),       # the same limit at V = 32
    (2, 8, 8, 25, 5, 17),        # instantiated <25, 8>, partial second class tile
    (2, 8, 9, 25, 7, 33),        # three class tiles, P = 7 (E * mid = 8j + 1: an odd split of the long tiles' K)
    (2, 8, 8, 25, 1, 1),         # instantiated <25, 8>, one node type, one edge class
    (2, 8, 3, 3, 2, 2),          # tiny graph
    (1, 8, 1, 2, 1, 1),          # degenerate graph
]
LIMIT_CASES = [(2, 16, 37, 25, 5, 15), (2, 8, 27, 32, 5, 15)]
# forward only (inference), past 128 samples and past the backward's range: mid = 40 fits one channel window, mid = 50 needs
# the two it takes at n <= 128 (refused at n > 128 while the window count followed the batch size)
FORWARD_CASES = [(129, 8, 40, 25, 5, 15), (129, 8, 50, 25, 5, 15)]
INSTANTIATED = {(V, mid) for V in (25, 17) for mid in (8, 16, 32)}


def case_seed(case):
    """check_dynadj's input seed"""
    return case[1] + case[2]


def case_id(case):
    return 'n{}-Ci{}-mid{}-V{}-P{}-E{}'.format(*case)


def dyn_inputs(n, Ci, mid, V, P, E, seed):
    """-> (t, node_type, edge_type): the dict of ``test_kernels_gpu._dyn_inputs`` (same keys, order and scales) for a graph
    of V joints with node_type = arange(V) % P and a random edge_type in [0, E) that holds every class when V*V >= E."""
    g = torch.Generator().manual_seed(seed)
    nt = (torch.arange(V) % P).to(torch.int32)
    et = torch.randint(0, E, (V * V,), generator=g)
    if V * V >= E:
        et[torch.randperm(V * V, generator=g)[:E]] = torch.arange(E)
    et = et.view(V, V).to(torch.int32)
    t = dict(
        xbar=torch.randn(n, Ci, V, generator=g),
        A=torch.randn(3, V, V, generator=g) * 0.02 + 0.04,
        alpha=torch.randn(3, generator=g) * 0.5, beta=torch.randn(3, generator=g) * 0.5,
        w1=torch.randn(2 * mid, Ci, generator=g) / Ci ** 0.5, b1=torch.randn(2 * mid, generator=g) * 0.1,
        w2=torch.randn(2 * mid, Ci, generator=g) / Ci ** 0.5, b2=torch.randn(2 * mid, generator=g) * 0.1,
        wse=torch.randn(mid * P, Ci, generator=g) / Ci ** 0.5, bse=torch.randn(mid * P, generator=g) * 0.1,
        we=torch.randn(E * mid, mid, generator=g) / mid ** 0.5, be=torch.randn(E * mid, generator=g) * 0.1)
    return t, nt, et


def dyn_cotangent(n, mid, V):
    """check_dynadj's output gradient"""
    return torch.randn(n, 3 * mid, V, V, generator=torch.Generator().manual_seed(7))


# ---- the kernel's launch arithmetic, restated (csrc/dynadj.hip) -------------------------------------------------------
LDS_MAX = 158 * 1024
CPC = 4                        # channels per thread of the backward's pass 1


def channel_groups(mid):
    return (mid + CPC - 1) // CPC


def ksplit(mid, V):
    """2: the long tiles of the subset-1 backward split K over the scratch; 1: they add straight into dX1 / dX2"""
    return 2 if V * V * (1 + channel_groups(mid)) >= 4 * mid * V else 1


def class_tiles(E):
    return (E + 15) >> 4


def lds_bytes(mid, V, E, backward, pm=None):
    """The carve in the comment above lds_G:  X1 [m][V] | X2 [m][V] | G [V][V] | col [V][2] | ET [V][V] | PQ [2][E][pm][V]
    (backward: | SC [V][V] | SCp [ceil(m/CPC)][V][V] | dX1 [m][V] | dX2 [m][V]), floats."""
    pm = mid if pm is None else pm
    f = mid * V + mid * V + V * V + 2 * V + V * V + 2 * E * pm * V
    if backward:
        f += V * V + channel_groups(mid) * V * V + mid * V + mid * V
    return 4 * f


def fwd_windows(n, mid, V, E):
    """channel windows per (sample, subset) of the forward; 0: no launch holds the shape"""
    split = 2 if (n <= 128 and mid >= 16) else 1
    if split == 1 and mid >= 2 and lds_bytes(mid, V, E, False) > LDS_MAX:
        split = 2
    return split if lds_bytes(mid, V, E, False, (mid + split - 1) // split) <= LDS_MAX else 0


def window_widths(mid, windows):
    return [mid * (z + 1) // windows - mid * z // windows for z in range(windows)]


def supported(n, mid, V, ld, E, backward):
    """dsgcn_dynadj_supported as a bool"""
    if n < 1 or mid < 1 or V < 1 or E < 1 or V > 32 or mid > 64 or ld < V:
        return False
    if backward:
        return lds_bytes(mid, V, E, True) <= LDS_MAX
    return fwd_windows(n, mid, V, E) > 0


def launch_lds(case):
    """-> (forward bytes, backward bytes) of a case's two launches"""
    n, _, mid, V, _, E = case
    w = fwd_windows(n, mid, V, E)
    return lds_bytes(mid, V, E, False, (mid + w - 1) // w), lds_bytes(mid, V, E, True)
