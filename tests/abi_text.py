"""Text parsers shared by test_rglue.py and test_abi_table.py: the declarations of include/sarlacc_amd.h and
the sarlacc_* calls of a source text, read without a compiler."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _split_args(s):
    """top-level comma split of an argument list"""
    out, depth, cur = [], 0, ""
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            out.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        out.append(cur.strip())
    return out


def _calls(text, prefix):
    """(name, [args]) for every `prefix...(` occurrence, with balanced parentheses"""
    res = []
    for m in re.finditer(r"\b(" + prefix + r"\w*)\s*\(", text):
        i, depth = m.end(), 1
        while depth:
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        res.append((m.group(1), _split_args(text[m.end():i - 1])))
    return res


def _type_text(decl):
    """'const int64_t* seq_off' -> ('const int64_t*', 'seq_off'): the declared type with single spaces and the
    stars attached to it, and the parameter's name"""
    m = re.fullmatch(r"(.*?)(\w+)", decl.strip(), flags=re.S)
    return re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), m.group(2)


def _header_decls():
    """name -> (return type text, [(parameter type text, parameter name), ...]) of every function the header declares"""
    text = _strip_comments(open(os.path.join(ROOT, "include", "sarlacc_amd.h")).read())
    decls = {}
    for name, args in _calls(text, "sarlacc_"):
        ret = re.search(r"([\w \t*]+?)\b" + name + r"\s*\(", text).group(1)
        decls[name] = (_type_text(ret + name)[0], [] if args == ["void"] else [_type_text(a) for a in args])
    return decls
