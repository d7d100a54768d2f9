"""collect_list / collect_set as a pure-Python model over lists of Python values: key tuple → kept values.

What it states (the semantics the engine follows; pinned on the reference's SQL test tables by tests/test_collect_cpu.py):
  NULL (None) inputs are dropped, and so are rows a FILTER rejects (keep[i] falsy — FALSE or NULL);
  a group whose rows are all dropped still exists, with an empty result; an ungrouped aggregate has the one group () even over no rows;
  collect_list keeps duplicates, in arrival order; collect_set keeps one of each distinct value (a Python set: no order);
  merging takes state rows (key, list) in input order — a NULL (None) or empty list adds nothing but makes its group exist — and concatenates the lists in
  that order, each in its own order; for a set it unites them.
Values are compared as Python compares them, so the model is for the in-scope set types (no floats: -0.0 == 0.0 and NaN != NaN there)."""


def collect_list(keys, values, keep=None, ungrouped=False):
    """keys[i]: the row's key tuple; → key → the kept values in arrival order"""
    out = {(): []} if ungrouped else {}
    for i, k in enumerate(keys):
        lst = out.setdefault(k, [])
        if values[i] is not None and (keep is None or keep[i]):
            lst.append(values[i])
    return out


def collect_set(keys, values, keep=None, ungrouped=False):
    return {k: set(v) for k, v in collect_list(keys, values, keep, ungrouped).items()}


def merge_list(state_rows, ungrouped=False):
    """state_rows: (key tuple, list or None) in input order; an element that is None is dropped"""
    out = {(): []} if ungrouped else {}
    for k, lst in state_rows:
        dst = out.setdefault(k, [])
        dst.extend(v for v in (lst or []) if v is not None)
    return out


def merge_set(state_rows, ungrouped=False):
    return {k: set(v) for k, v in merge_list(state_rows, ungrouped).items()}


def state_rows(state):
    """a model result as state rows, for merging"""
    return [(k, list(v)) for k, v in state.items()]
