"""The Python binding's public surface, pinned: every public name of grail_hip with its call signature, its value or its
kind, and every public method of its classes, against tests/golden/binding_surface.txt.  Needs no built library.

The file was written by `python tests/test_binding_surface.py > tests/golden/binding_surface.txt` on the commit before the
binding was split into _abi / host / device; it is regenerated the same way when the surface is changed on purpose."""
import ast
import inspect
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_surface.txt")
# values that depend on where the package lies: listed by type only
BY_TYPE_ONLY = ("LIB_PATH",)


def _methods(cls):
    for name in sorted(dir(cls)):
        attr = getattr(cls, name)
        if not name.startswith("_") and (inspect.isfunction(attr) or inspect.ismethod(attr)):
            yield f"{cls.__name__}.{name}{inspect.signature(attr)}"


def surface_listing(G):
    lines = []
    for name in sorted(vars(G)):
        value = getattr(G, name)
        if name.startswith("_") or isinstance(value, types.ModuleType):
            continue
        if inspect.isclass(value):
            lines.append(f"{name}: class")
            lines.extend(_methods(value))
        elif callable(value):
            lines.append(f"{name}{inspect.signature(value)}")
        elif name in BY_TYPE_ONLY:
            lines.append(f"{name}: {type(value).__name__}")
        else:                                       # the int / float / str constants; EXPORTS and PHONEME_DTYPE too
            lines.append(f"{name} = {value!r}")
    return "".join(line + "\n" for line in sorted(lines))


def test_public_surface_is_what_the_golden_file_lists():
    import grail_hip as G
    got, want = surface_listing(G), open(GOLDEN).read()
    if got != want:
        g, w = set(got.splitlines()), set(want.splitlines())
        raise AssertionError("surface changed\n  gone: " + "\n        ".join(sorted(w - g)) +
                             "\n  new:  " + "\n        ".join(sorted(g - w)))


def test_every_address_handed_to_the_library_is_of_a_named_array():
    """_ptr(a) gives a plain number: an array made in the argument itself (`_ptr(np.ascontiguousarray(...))`, `_ptr(_marks(...))`)
    is released before the library reads it.  Every _ptr call in the package takes a name, and so does every
    `<expr>.ctypes.data`: the array is a local that lives across the call."""
    pkg = os.path.join(ROOT, "grail-rs_amd", "grail_hip")
    bad = []
    for fname in sorted(f for f in os.listdir(pkg) if f.endswith(".py")):
        for node in ast.walk(ast.parse(open(os.path.join(pkg, fname)).read())):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "_ptr":
                holder = node.args[0]
            elif isinstance(node, ast.Attribute) and node.attr == "ctypes":
                holder = node.value
            else:
                continue
            if not isinstance(holder, ast.Name):
                bad.append(f"{fname}:{node.lineno}")
    assert not bad, bad


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "grail-rs_amd"))
    import grail_hip
    sys.stdout.write(surface_listing(grail_hip))
