"""The routing policy of ``FlatIndex`` on stated corpus facts, without a device: a real ``ScanRouting`` for the policy
tests of the index (``n`` rows, largest row norm ``cmax``, ``complete`` = the scans whose image already holds every row)."""
from sessionsimilaritysearch_amd import index as ix
from sessionsimilaritysearch_amd.routing import ScanRouting


def make_routing(d, metric="ip", dtype="f32", scan=None, n=1000, cmax=1.0, pad_scan=False, complete=()):
    return ScanRouting(d, metric, dtype, scan, pad_scan, fmt=ix._FORMATS[dtype], ntotal=n, max_norm=cmax, complete=complete)
