"""jsp_explain without a GPU: the header declares it, the ctypes struct has the
ABI's size, a NULL engine is JSP_EINVAL, and the host mirror's
placement.explainMessage (a pure JSON method, no engine call) writes the
format DESIGN.md §6 fixes."""
import ctypes
import os
import re

from jobset_amd import host, native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_jsp_explain():
    src = open(os.path.join(ROOT, "include", "jsplace.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"^int\s+jsp_explain\s*\(\s*jsp_engine\s*\*\s*e\s*,\s*jsp_class_explain\s*\*\s*out\s*,"
                     r"\s*uint32_t\s+n_classes\s*\)\s*;", src, flags=re.M)
    assert "typedef struct jsp_class_explain" in src
    assert "#define JSP_ABI_VERSION 7" in src  # additive: a caller detects it by symbol


def test_struct_size_is_104():
    assert ctypes.sizeof(native.JspClassExplain) == 104
    assert native.JspClassExplain.rows_insufficient.offset == 32
    assert native.JspClassExplain.domains.offset == 80
    assert native.JspClassExplain.best_short_domain.offset == 100


def test_null_engine_is_einval():
    out = (native.JspClassExplain * 1)()
    assert native.lib().jsp_explain(None, out, 1) == native.JSP_EINVAL


def counts(**kw):
    c = dict(rows=0, rowsSelector=0, rowsTaint=0, rowsNoCapacity=0, rowsInsufficient=[0, 0, 0], rowsFit=0,
             rowsOccupied=0, domains=0, domOccupied=0, domShort=0, domFeasible=0, bestShortCap=0,
             bestShortDomain=-1)
    c.update(kw)
    return c


RES = ["cpu", "memory", "amd.com/gpu"]


def test_message_all_clauses():
    c = counts(rows=160, rowsSelector=40, rowsTaint=8, rowsNoCapacity=20, rowsInsufficient=[0, 0, 20], rowsFit=92,
               rowsOccupied=32, domains=10, domOccupied=2, domShort=5, domFeasible=3, bestShortCap=12,
               bestShortDomain=7)
    assert host.explainMessage(c, "rack", 16, RES, "rack-7") == (
        "3/10 rack domains can hold a job of 16 pods: 2 held by another exclusive job, "
        "5 too small (largest, rack-7, fits 12 pods). "
        "160 nodes: 40 didn't match the node selector, 8 had untolerated taints, "
        "20 lacked resources (Insufficient amd.com/gpu: 20), 92 fit at least one pod.")


def test_message_omits_zero_clauses_and_empty_groups():
    c = counts(rows=12, rowsFit=12, domains=4, domFeasible=4)
    assert host.explainMessage(c, "cloud.google.com/gke-nodepool", 3, RES) == (
        "4/4 cloud.google.com/gke-nodepool domains can hold a job of 3 pods. 12 nodes: 12 fit at least one pod.")
    c = counts(rows=32, rowsTaint=32, domains=8, domShort=8, bestShortCap=0, bestShortDomain=0)
    assert host.explainMessage(c, "rack", 4, RES, "rack-0") == (
        "0/8 rack domains can hold a job of 4 pods: 8 too small (largest, rack-0, fits 0 pods). "
        "32 nodes: 32 had untolerated taints.")
    c = counts(domains=2, domFeasible=0, domOccupied=2)
    assert host.explainMessage(c, "zone", 1, RES) == (
        "0/2 zone domains can hold a job of 1 pods: 2 held by another exclusive job. 0 nodes.")


def test_message_without_a_short_domain_has_no_largest():
    c = counts(rows=48, rowsSelector=16, rowsFit=32, rowsOccupied=16, domains=3, domOccupied=1, domFeasible=2)
    msg = host.explainMessage(c, "rack", 16, RES)
    assert msg == ("2/3 rack domains can hold a job of 16 pods: 1 held by another exclusive job. "
                   "48 nodes: 16 didn't match the node selector, 32 fit at least one pod.")
    assert "largest" not in msg and "(" not in msg


def test_message_names_two_short_resources():
    c = counts(rows=10, rowsNoCapacity=6, rowsInsufficient=[3, 5, 0], rowsFit=4, domains=1, domShort=1,
               bestShortCap=4, bestShortDomain=0)
    assert host.explainMessage(c, "rack", 8, RES, "r0") == (
        "0/1 rack domains can hold a job of 8 pods: 1 too small (largest, r0, fits 4 pods). "
        "10 nodes: 6 lacked resources (Insufficient cpu: 3, Insufficient memory: 5), 4 fit at least one pod.")
