"""A plain restatement of the anchored null's tree (include/rnacode_hip.h, "The anchored null"): T rooted at a new node on the reference
tip's edge, at distance 0 from the tip.  Independent of the library's anchor_tree (rc_host.cpp): it works on a nested structure parsed from
the Newick text, and the tests compare both with trees written out by hand."""
from typing import List, Optional


class Node:
    def __init__(self, name: Optional[str] = None, kids: Optional[List["Node"]] = None, length: Optional[float] = None):
        self.name, self.kids, self.length, self.up = name, kids or [], length, None
        for k in self.kids:
            k.up = self


def parse(text: str) -> Node:
    """Newick with a length on every node but the root; labels of inner nodes are not kept."""
    pos = text.index("(")

    def subtree():
        nonlocal pos
        if text[pos] == "(":
            pos += 1
            kids = [subtree()]
            while text[pos] == ",":
                pos += 1
                kids.append(subtree())
            assert text[pos] == ")", text[pos:]
            pos += 1
            while text[pos] not in ":,);":
                pos += 1
            node = Node(kids=kids)
        else:
            at = pos
            while text[pos] not in ":,)":
                pos += 1
            node = Node(name=text[at:pos].strip())
        if text[pos] == ":":
            at = pos = pos + 1
            while text[pos] not in ",);":
                pos += 1
            node.length = float(text[at:pos])
        return node

    return subtree()


def tips(node: Node) -> List[Node]:
    return [node] if not node.kids else [t for k in node.kids for t in tips(k)]


def anchor(root: Node, ref_name: str) -> Node:
    (ref,) = [t for t in tips(root) if t.name == ref_name]

    def entered(x: Node, frm: Node, length: float) -> Node:
        """x as it hangs below the neighbour it is entered from."""
        if not x.kids:
            return Node(name=x.name, length=length)
        kids = [entered(c, x, c.length) for c in x.kids if c is not frm]   # its children in their order, minus the one it is entered from
        if x.up is not None and frm is not x.up:
            kids.append(behind(x))                                         # then its former parent
        return Node(kids=kids, length=length)

    def behind(x: Node) -> Node:
        """What lies behind x's parent, on x's own former branch; a two-child root is dissolved: its other child, the two branches summed."""
        p = x.up
        if p.up is None and len(p.kids) == 2:
            (w,) = [k for k in p.kids if k is not x]
            return entered(w, p, x.length + w.length)
        return entered(p, x, x.length)

    return Node(kids=[Node(name=ref.name, length=0.0), behind(ref)])


def write(node: Node) -> str:
    def text(n: Node) -> str:
        s = n.name if not n.kids else "(" + ",".join(text(k) for k in n.kids) + ")"
        return s if n.length is None else s + ":%.17g" % n.length
    return text(node) + ";"


def anchored_newick(newick: str, ref_name: str) -> str:
    return write(anchor(parse(newick), ref_name))


def shape(node: Node):
    """The tree as nested tuples (name or children, length as a double): topology, child order and lengths compare exactly."""
    return (node.name if not node.kids else tuple(shape(k) for k in node.kids), node.length)
