"""The argument checks and the statistic that the two engines, the sampler and the utilities share: one copy of each."""
import numpy as np


def check_kernel_name(kernel):
    if kernel not in ("rbf", "imq"):
        raise ValueError("kernel must be \"rbf\" or \"imq\", got %r" % (kernel,))


def check_engine_switches(kernel, h2, median_every):   # both engines' first checks, in this order -> is h2 "median"?
    check_kernel_name(kernel)
    if kernel == "imq" and h2 is None:
        raise ValueError("kernel=\"imq\": the IMQ kernel exists as a streaming step only (no stored-D path); pass h2= "
                         "(h2=\"median\" for the median heuristic's bandwidth)")
    stream_median = isinstance(h2, str) and h2 == "median"
    if isinstance(median_every, bool) or not isinstance(median_every, int) or median_every < 1:
        raise ValueError("median_every must be an integer >= 1, got %r" % (median_every,))
    if median_every != 1 and not stream_median:
        raise ValueError("median_every= is the refresh period of h2=\"median\" (the streaming step at the median "
                         "heuristic's bandwidth); it is not supported on any other engine")
    return stream_median


def positive_float(value, name, what, long_name=None):   # what: the forms the caller accepts.  No bool, no string
    try:
        x = None if isinstance(value, (bool, np.bool_, str)) else float(value)
    except (TypeError, ValueError):
        x = None
    if x is None:
        raise ValueError("%s must be %s, got %r" % (name, what, value))
    if not 0.0 < x < float("inf"):      # (false for a NaN too)
        raise ValueError("%s must be positive and finite, got %r" % (long_name or name, value))
    return x


def bandwidth_to_h2(bandwidth, what):
    """a bandwidth= argument (a float h, or "median") -> the h2= argument of a streaming engine (h^2, or "median")"""
    if isinstance(bandwidth, str) and bandwidth == "median":
        return "median"
    h = positive_float(bandwidth, "bandwidth", what)
    return h * h


def ksd_statistic(S, S_diag, n, statistic):
    """KSD^2, the U- ("u") or V-statistic ("v"), from S = sum_ij u_ij and S_diag = sum_i u_ii over n particles; no host sync"""
    n = float(n)
    if statistic == "u" and n < 2:
        raise ValueError("n = 1: the U-statistic needs at least two particles (statistic='v' is defined)")
    if statistic not in ("u", "v"):
        raise ValueError("statistic must be 'u' or 'v'")
    return S / (n * n) if statistic == "v" else (S - S_diag) / (n * (n - 1.0))
