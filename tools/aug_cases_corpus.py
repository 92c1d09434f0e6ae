"""Writes the input of tools/aug_host_check.cpp: the case list of tests/aug_cases.py (a record and a tile pair per case, at every size).

    python tools/aug_cases_corpus.py cases.bin
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main(path):
    import aug_cases as AC

    with open(path, "wb") as f:
        f.write(AC.corpus_blob())
    print(f"{len(AC.corpus())} cases -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
