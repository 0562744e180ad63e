"""Generates tests/golden/kdtree_ref_digests.json (run where oracle/_ref/libkdtree_ref.so is built by oracle/Makefile).

For every input of tests/test_oracle_dbscan.py's reference-tree tests (range queries of every point, DBSCAN Run() on top of
the kd_* ABI, the arc slices) the results of the REFERENCE's own kd-tree are recorded as one SHA-1 digest, after being
asserted equal to the fully restated oracle.  Fixtures are data only: lists of hex digests.

    python tests/golden/make_kdtree_ref_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
import test_oracle_dbscan as T  # noqa: E402


def main():
    assert O.have_ref_kdtree(), "oracle/_ref/libkdtree_ref.so is not built"
    out = {"range_query": {}, "driver": {}, "arc_slices": []}
    for seed in range(6):
        out["range_query"][str(seed)] = []
        for xy, eps in T.range_query_cases(seed):
            o2, i2 = O.range_query_all(xy, eps, kdapi=True)
            o1, i1 = O.range_query_all(xy, eps)
            assert (o1 == o2).all() and (i1 == i2).all()
            out["range_query"][str(seed)].append(T._digest(o2, i2))
    for seed in range(4):
        out["driver"][str(seed)] = []
        for xy, eps, minpts in T.driver_cases(seed):
            rc, lab, n, cl = O.dbscan(xy, eps, minpts, kdapi=True, with_members=True)
            assert rc == 0 and T._dbscan_digest(*O.dbscan(xy, eps, minpts, with_members=True)) == T._dbscan_digest(rc, lab, n, cl)
            out["driver"][str(seed)].append(T._dbscan_digest(rc, lab, n, cl))
    for xy in T.arc_cases():
        rc, lab, n = O.dbscan(xy, 4.0, 2, kdapi=True)
        assert T._dbscan_digest(*O.dbscan(xy, 4.0, 2)) == T._dbscan_digest(rc, lab, n)
        out["arc_slices"].append(T._dbscan_digest(rc, lab, n))
    path = os.path.join(HERE, "kdtree_ref_digests.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("%s: %d digests, %.1f KB" % (path, sum(len(v) for v in out["range_query"].values()) + sum(len(v) for v in out["driver"].values())
                                       + len(out["arc_slices"]), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
