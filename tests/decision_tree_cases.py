"""Cases of the decision-tree tests; nothing here comes from the product.  An integer model of every method of the circuit with the
circuit's floors (signed Python integers at scale 2^63), a float model of a textbook CART Gini split, the data sets — each built for one
edge — and the inference inputs.

The training shape is the smallest that reaches every branch: 4 samples x 2 features, 2 classes, max_depth 2, min_size 1 — two features
keep data_slot = 1 and the stride live, depth 2 runs the inner-node and the last-layer branch, the layer-1 queue holds a left and a right
mask.  It is 71 757 cells, 18 gate + 5 lookup-advice columns at DEGREE 12 / LOOKUP_BITS 11, the smallest DEGREE that holds it (11 / 10
needs more than 32 gate columns).  One set differs: with max_depth 2 the only node the leaf-by-size selects act on is the root, which
holds all four samples, so no min_size below 4 makes a leaf by size there; the min_size = 2 set therefore runs at max_depth 3, where the
layer-1 nodes hold two samples each — 167 000 cells, DEGREE 13 / LOOKUP_BITS 12."""
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
P = 63
ONE = 1 << P
MASK_CLS = 255
GAP = 1 << (P - 40)  # 2^-40 at scale 2^63


def q(x: float) -> int:
    """round(|x| 2^P), halves away from zero, signed"""
    m = int(abs(x) * float(ONE) + 0.5)
    return -m if x < 0 else m


def to_field(s: int) -> int:
    return s % R


def field_inputs(inputs):
    return type(inputs)(field_inputs(v) for v in inputs) if isinstance(inputs, (list, tuple)) else to_field(inputs)


# ---- the integer model ----------------------------------------------------------------------------------------------------------------------
def ref_inference(tree, x, max_path_len: int) -> tuple:
    """-> (class, the node the path ends at).  An index beyond a list selects 0"""
    at = lambda values, i: values[i] if 0 <= i < len(values) else 0
    node = 0
    for _ in range(max_path_len):
        slot, split, left, right = (at(tree, node * 5 + i) for i in range(4))
        node = left if at(x, slot) - split < 0 else right  # a zero difference is not negative: right
    return at(tree, node * 5 + 4), node


def ref_gini(xs, ys, masks, slot: int, num_feature: int, num_class: int, split: int) -> int:
    cnt = group1 = group2 = 0
    in1, in2 = [0] * num_class, [0] * num_class
    for x, y, m in zip(xs[slot::num_feature], ys, masks):
        cnt += m
        less = int(x - split < 0)
        group1 += less * m
        group2 += (1 - less) * m
        for c in range(num_class):
            in1[c] += int(y == c) * less * m
            in2[c] += int(y == c) * (1 - less) * m
    cnt = cnt or 1  # no sample: one
    size1, size2 = group1 * ONE + 1, group2 * ONE + 1  # the epsilon

    def group(counts, size):
        g = ONE
        for n in counts:
            p = (n * ONE * ONE) // size
            g -= (p * p) // ONE
        return (g * (size // cnt)) // ONE

    return ONE if cnt < 2 else group(in1, size1) + group(in2, size2)  # the leaf fix


def ref_candidates(xs, ys, masks, num_feature: int, num_class: int) -> list:
    """[(gini, slot, split)] in the order get_split tries them: every sample x feature, the candidate's own mask multiplied in"""
    return [(ref_gini(xs, ys, [m * masks[i] for m in masks], j, num_feature, num_class, xs[i * num_feature + j]), j, xs[i * num_feature + j])
            for i in range(len(ys)) for j in range(num_feature)]


def ref_get_split(xs, ys, masks, num_feature: int, num_class: int) -> tuple:
    best, best_slot, best_split = ONE, 0, xs[0]
    for g, slot, split in ref_candidates(xs, ys, masks, num_feature, num_class):
        if g < best:  # strictly: the first best wins
            best, best_slot, best_split = g, slot, split
    return best_slot, best_split


def ref_common_cls(ys, masks, num_class: int) -> int:
    counts = [sum(m for y, m in zip(ys, masks) if y == c) for c in range(num_class)]
    out = most = 0
    for c, n in enumerate(counts):
        if most < n:  # strictly: the lowest class of equals, 0 for no sample
            out, most = c, n
    return out


def ref_train(xs, ys, num_feature: int, num_class: int, max_depth: int, min_size: int, nodes_seen: list = None) -> list:
    """the flat tree; nodes_seen, if given, collects (masks, candidates) per node"""
    queue, tree = [[1] * len(ys)], []
    for layer in range(max_depth):
        for node_idx in range(len(queue)):
            masks = queue.pop(0)
            leaf = sum(masks) < min_size + 1
            if nodes_seen is not None:
                nodes_seen.append((masks, ref_candidates(xs, ys, masks, num_feature, num_class)))
            slot, split = ref_get_split(xs, ys, masks, num_feature, num_class)
            lefts = [int(xs[i * num_feature + slot] - split < 0) for i in range(len(ys))]
            cls = ref_common_cls(ys, masks, num_class)
            cur = 2 ** layer - 1 + node_idx
            if layer < max_depth - 1:
                queue.append([m * l for m, l in zip(masks, lefts)])
                queue.append([m * (1 - l) for m, l in zip(masks, lefts)])
                tree += [0, 0, cur, cur, cls] if leaf else [slot, split, 2 * cur + 1, 2 * cur + 2, MASK_CLS]
            else:
                tree += [0, 0, cur, cur, cls]
    return tree


# ---- the float model: a textbook CART split ----------------------------------------------------------------------------------------------------
TIE = 2.0 ** -41  # half the gap the integer model asserts between distinct impurities: below it two floats are one value


def cart_impurity(rows, labels, members, feature: int, threshold: float, num_class: int) -> float:
    """the size-weighted Gini impurity 1 - sum p_c^2 of the two sides of `x[feature] < threshold` among the members"""
    total = 0.0
    for side in ([s for s in members if rows[s][feature] < threshold], [s for s in members if not rows[s][feature] < threshold]):
        if side:
            shares = [sum(1 for s in side if labels[s] == c) / len(side) for c in range(num_class)]
            total += len(side) / len(members) * (1.0 - sum(p * p for p in shares))
    return total


def cart_train(rows, labels, num_class: int, max_depth: int, min_size: int) -> list:
    """a complete tree, breadth first, as rows (feature, threshold, left, right, class): every member x feature is a candidate threshold,
    the first of the least impurity is taken; fewer than two members have no split to choose and pass on by feature 0 at sample 0;
    a node of at most min_size members, and every node of the last layer, is a leaf of its most common class (the lowest of equals)"""
    queue, tree = [list(range(len(rows)))], []
    for layer in range(max_depth):
        for node_idx in range(len(queue)):
            members = queue.pop(0)
            feature, threshold, best = 0, rows[0][0], 1.0
            if len(members) >= 2:
                for s in members:
                    for f in range(len(rows[0])):
                        g = cart_impurity(rows, labels, members, f, rows[s][f], num_class)
                        if g < best - TIE:
                            feature, threshold, best = f, rows[s][f], g
            counts = [sum(1 for s in members if labels[s] == c) for c in range(num_class)]
            cls = counts.index(max(counts)) if members else 0
            cur = 2 ** layer - 1 + node_idx
            if layer < max_depth - 1:
                queue.append([s for s in members if rows[s][feature] < threshold])
                queue.append([s for s in members if not rows[s][feature] < threshold])
                tree.append((0, 0.0, cur, cur, cls) if len(members) <= min_size else (feature, threshold, 2 * cur + 1, 2 * cur + 2, MASK_CLS))
            else:
                tree.append((0, 0.0, cur, cur, cls))
    return tree


def quantised_tree(rows) -> list:
    """cart_train's rows as the flat integer tree"""
    return [v for f, t, left, right, cls in rows for v in (f, q(t), left, right, cls)]


# ---- the training sets ----------------------------------------------------------------------------------------------------------------------------
NUM_FEATURE, NUM_CLASS, MAX_DEPTH, MIN_SIZE = 2, 2, 2, 1
TRAIN_K, TRAIN_LOOKUP_BITS = 12, 11
DEEP_K, DEEP_LOOKUP_BITS = 13, 12  # of the one set at max_depth 3


class DataSet:
    def __init__(self, name, rows, labels, ties: bool = False, max_depth: int = MAX_DEPTH, min_size: int = MIN_SIZE):
        self.name, self.rows, self.labels, self.ties = name, rows, labels, ties
        self.max_depth, self.min_size = max_depth, min_size
        self.k, self.lookup_bits = (TRAIN_K, TRAIN_LOOKUP_BITS) if max_depth == MAX_DEPTH else (DEEP_K, DEEP_LOOKUP_BITS)
        self.xs, self.ys = [q(v) for row in rows for v in row], list(labels)
        self.nodes = []
        self.tree = ref_train(self.xs, self.ys, NUM_FEATURE, NUM_CLASS, max_depth, min_size, self.nodes)

    @property
    def inputs(self):
        """the closure's inputs, in the field"""
        return field_inputs((self.xs, self.ys))

    @property
    def public(self):
        return field_inputs(self.tree)

    def node(self, i: int) -> list:
        return self.tree[5 * i:5 * i + 5]


DATA_SETS = [
    DataSet("feature 0 separates", [[1.25, 5.0], [2.771244718, 7.5], [3.5, 6.0], [4.0, 8.25]], [0, 0, 1, 1]),
    DataSet("feature 1 separates", [[5.0, 1.25], [7.5, 2.771244718], [6.0, 3.5], [8.25, 4.0]], [0, 0, 1, 1]),
    DataSet("values equal to the split", [[1.0, 0.5], [1.5, 1.5], [2.0, 0.5], [2.0, 1.5]], [0, 0, 1, 1]),
    DataSet("identical samples, different labels", [[1.5, 1.0], [1.5, 1.0], [2.5, 3.0], [3.25, 2.0]], [0, 1, 1, 1]),
    DataSet("negative values", [[-3.5, 0.25], [-2.5, -2.0], [-1.25, -0.75], [-0.5, -4.5]], [1, 1, 0, 0]),
    DataSet("all labels equal", [[1.0, 3.0], [1.0, 4.0], [2.0, 3.0], [2.0, 4.0]], [1, 1, 1, 1]),
    DataSet("equal impurities on two features", [[1.0, 1.0], [2.0, 2.0], [3.0, 3.0], [4.0, 4.0]], [0, 0, 1, 1], ties=True),
    DataSet("equal impurities, mirrored groups", [[1.0, 9.0], [2.0, 8.0], [3.0, 7.0], [4.0, 6.0]], [0, 1, 1, 1], ties=True),
    DataSet("leaves by size", [[1.0, 5.0], [2.0, 5.0], [3.0, 5.0], [4.0, 5.0]], [0, 0, 1, 0], max_depth=3, min_size=2),
]
BY_NAME = {d.name: d for d in DATA_SETS}
SHALLOW = [d for d in DATA_SETS if d.max_depth == MAX_DEPTH]
TRAIN_DUMMY = DataSet("dummy", [[0.5, 0.5], [1.5, 2.5], [2.5, 1.5], [3.5, 3.5]], [0, 1, 0, 1])
PROVEN = ["feature 1 separates", "negative values", "all labels equal"]  # the three proven whole; the first again under the other keys


def _check_data_sets():
    """each set is what it is named for, in the integer model alone; without engineered ties the best and the second-best distinct
    impurity of every node are more than 2^-40 apart, far above the roundings of a 63-bit fraction, which is what lets the float model
    be compared tree for tree"""
    for d in DATA_SETS:
        if not d.ties:
            for masks, candidates in d.nodes:
                distinct = sorted({g for g, _, _ in candidates})
                assert len(distinct) < 2 or distinct[1] - distinct[0] > GAP, (d.name, masks, distinct[:2])
    by = BY_NAME
    assert by["feature 0 separates"].node(0) == [0, q(3.5), 1, 2, MASK_CLS] and by["feature 1 separates"].node(0) == [1, q(3.5), 1, 2, MASK_CLS]
    for name in ("feature 0 separates", "feature 1 separates"):
        assert by[name].node(1) == [0, 0, 1, 1, 0] and by[name].node(2) == [0, 0, 2, 2, 1]
    d = by["values equal to the split"]
    assert d.node(0) == [0, q(2.0), 1, 2, MASK_CLS] and d.nodes[1][0] == [1, 1, 0, 0] and d.nodes[2][0] == [0, 0, 1, 1]  # both 2.0 go right
    d = by["identical samples, different labels"]
    assert d.xs[0:2] == d.xs[2:4] and d.ys[0] != d.ys[1] and sorted(d.nodes[1][0] + d.nodes[2][0]) == [0] * 4 + [1] * 4
    assert d.nodes[1][0][0] == d.nodes[1][0][1]  # no split parts them
    d = by["negative values"]
    assert d.node(0)[1] < 0 and d.node(0)[4] == MASK_CLS
    d = by["all labels equal"]
    assert d.node(0) == [0, q(1.0), 1, 2, MASK_CLS] and d.nodes[1][0] == [0] * 4 and d.node(1) == [0, 0, 1, 1, 0] and d.node(2) == [0, 0, 2, 2, 1]
    assert all(g == ONE for g, _, _ in d.nodes[1][1])  # the count of zero replaced by one, then the leaf fix
    d = by["equal impurities on two features"]
    g = [c[0] for c in d.nodes[0][1]]
    assert g[4] == g[5] == min(g) and d.node(0)[:2] == [0, q(3.0)]  # sample 2's two features: feature 0 comes first
    d = by["equal impurities, mirrored groups"]
    g = [c[0] for c in d.nodes[0][1]]
    assert g[1] == g[2] == min(g) and g[0] > g[1] and d.node(0)[:2] == [1, q(9.0)]  # (sample 0, feature 1) before (sample 1, feature 0)
    d = by["leaves by size"]
    assert [sum(m) for m, _ in d.nodes[1:3]] == [2, 2] and d.node(1) == [0, 0, 1, 1, 0] and d.node(2) == [0, 0, 2, 2, 0]
    assert ref_train(d.xs, d.ys, NUM_FEATURE, NUM_CLASS, 3, 1)[10:15] == [0, q(4.0), 5, 6, MASK_CLS]  # at min_size 1 node 2 would split
    assert len({tuple(d.tree) for d in SHALLOW} | {tuple(TRAIN_DUMMY.tree)}) >= 7


_check_data_sets()

# gini and common_cls at three classes: (xs, ys, masks, slot, num_feature, num_class, split) on 5 samples x 2 features
_X3 = [q(v) for row in [[0.5, -1.0], [1.5, 2.0], [2.5, -3.0], [3.5, 4.0], [4.5, 0.0]] for v in row]
_Y3 = [0, 1, 2, 1, 2]
GINI_3 = [(_X3, _Y3, [1, 1, 1, 1, 1], 0, 2, 3, q(2.5)), (_X3, _Y3, [1, 1, 1, 1, 1], 1, 2, 3, q(0.0)), (_X3, _Y3, [1, 0, 1, 1, 0], 0, 2, 3, q(3.5)),
          (_X3, _Y3, [0, 0, 0, 0, 0], 1, 2, 3, q(2.0)), (_X3, _Y3, [0, 0, 1, 0, 0], 0, 2, 3, q(0.5)), (_X3, _Y3, [1, 1, 1, 1, 1], 0, 2, 3, q(0.5))]
COMMON_3 = [(_Y3, [1, 1, 1, 1, 1]), (_Y3, [1, 0, 1, 0, 0]), (_Y3, [0, 0, 0, 0, 0]), (_Y3, [0, 0, 1, 0, 1]), ([2, 2, 1, 1, 0], [1, 1, 1, 1, 1])]

# ---- inference ----------------------------------------------------------------------------------------------------------------------------------
INFERENCE_K, INFERENCE_LOOKUP_BITS = 9, 8  # 7625 cells: 16 gate columns and one lookup-advice column
TREE = [0, q(1.3), 1, 2, MASK_CLS,
        1, q(-3.5), 3, 4, MASK_CLS,
        0, 0, 2, 2, 1,
        0, 0, 3, 3, 1,
        0, 0, 4, 4, 0,
        0, 0, 5, 5, 0,
        0, 0, 6, 6, 1]
MAX_PATH_LEN = 3
# (x, class, the leaf reached): one per reachable leaf — the second ends after one step and walks its leaf's self-loop twice —, and two
# that sit on a split exactly: a zero difference is not negative
INFERENCE_INPUTS = [([q(-1.2), q(0.1)], 0, 4), ([q(2.1), q(3.2)], 1, 2), ([q(0.0), q(-4.0)], 1, 3), ([q(1.3), q(-9.0)], 1, 2), ([q(1.0), q(-3.5)], 0, 4)]
INFERENCE_DUMMY = [q(0.5), q(0.5)]
ONE_NODE_TREE = [0, 0, 0, 0, 1]
for _x, _cls, _leaf in INFERENCE_INPUTS:
    assert ref_inference(TREE, _x, MAX_PATH_LEN) == (_cls, _leaf)
assert {leaf for _, _, leaf in INFERENCE_INPUTS} == {2, 3, 4} and ref_inference(ONE_NODE_TREE, [q(-1.2), q(0.1)], MAX_PATH_LEN) == (1, 0)

# the reference's two data sets and what the integer model makes of them at its sizes (max_depth 4): the example's output
EXAMPLE_X = [[2.771244718, 1.784783929], [1.0, 1.0], [3.0, 2.0], [3.0, 2.0], [2.0, 2.0], [7.0, 3.0], [9.00220326, 3.339047188], [7.444542326, 0.476683375],
             [10.12493903, 3.234550982], [6.642287351, 3.319983761]]
EXAMPLE_Y = [1, 0, 0, 1, 0, 1, 1, 0, 1, 1]
EXAMPLE_DUMMY_X = [[2.771244718, 1.784783929], [1.728571309, 1.169761413], [3.678319846, 2.81281357], [3.961043357, 2.61995032], [2.999208922, 2.209014212],
                   [7.497545867, 3.162953546], [9.00220326, 3.339047188], [7.444542326, 0.476683375], [10.12493903, 3.234550982], [6.642287351, 3.319983761]]
EXAMPLE_DUMMY_Y = [0, 0, 0, 0, 0, 1, 1, 1, 1, 1]


def example_tree(rows, labels) -> list:
    return ref_train([q(v) for row in rows for v in row], list(labels), 2, 2, 4, 1)
