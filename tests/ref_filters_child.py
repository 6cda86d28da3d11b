"""Runs the compiled reference (oracle/_ref) over the filter table of tests/filter_reference.py and prints one JSON line per
filter: the digests tests/golden/ref_filters.json pins.  Started as a child process under a time limit by
tests/test_filter_reference.py and tests/golden/make_golden.py: outside its domain the reference can fail to return.
usage: python tests/ref_filters_child.py omp|serial"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import filter_reference as F  # noqa: E402
from oracle import oracle as O  # noqa: E402


def main():
    which = sys.argv[1]
    for name in F.FILTERS:
        d = F.digests(name, lambda x, opts: O.ref_encode_chunk(x, opts, which), lambda w, opts: O.ref_decode_chunk(w, opts, which))
        if d:
            print(json.dumps(d), flush=True)


if __name__ == "__main__":
    main()
