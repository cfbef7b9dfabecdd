"""What a C header of include/ declares, for the tests that hold a binding's SIGNATURES against it.  A helper module (like
tests/_guarded.py), not a test file."""
import os
import re

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def declared_symbols(key: str) -> set:
    """Every `<prefix>_name(` of the library's header outside comments: the functions it declares (a type is never followed by a
    parenthesis; the prose of the comments, which names functions freely, is stripped first)."""
    from anystereo._srchash import LIBRARIES
    row = LIBRARIES[key]
    text = open(os.path.join(ROOT, row.header)).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return set(re.findall(r"\b(%s_[a-z0-9_]+)\s*\(" % row.prefix, text))
