"""DecisionTreeChip over FixedPointChip, after the reference's src/gadget/decision_tree.rs, name for name and call for call: inference
down a tree given as constants, and CART training by the Gini impurity — every sample x feature a candidate split, every candidate a Gini
over the whole data set under the node's masks —, and the two closures of its examples/decision_tree.rs as the scaffold takes them.
Every input of a closure is an integer — the callers quantise (FixedPointChip.quantization) before `prove` — so both record as witness
programs.  The circuit is comparisons: every `data < split` is an is_neg (two 254-bit divisions and an inversion), every
select_from_idx a row of is_equal.  A tree is a flat list, five entries a node: data_slot, split, left, right, cls; an inner node's cls
is MASK_CLS, a leaf points at itself.

Written from the algorithm; what is restated is the sequence of builder calls, which fixes the circuit — the reference's quirks with it:
the feature column of `gini` is dataset_x[data_slot::num_feature]; a count of zero samples is replaced by one; both scaled group sizes
carry a + 1 so that nothing divides by zero; a node of fewer than two samples gets the impurity 1.0."""
from .fixed_point import FixedPointChip
from .flex import Constant

PRECISION_BITS = 63
MASK_CLS = 255


class DecisionTreeChip:
    def __init__(self, lookup_bits: int = None):
        self.chip = FixedPointChip(PRECISION_BITS, lookup_bits)
        self.lookup_bits = lookup_bits

    def inference(self, ctx, tree, x, max_path_len: int):
        """the class of x (values: the closure's inputs) under `tree` (integers, constants of the circuit), max_path_len steps from the
        root; a leaf's children are the leaf, so a path that ends early stays where it ended"""
        tree = [Constant(v) for v in tree]
        x = list(x)
        node_idx = ctx.add(Constant(0), Constant(0))
        x_advice = [ctx.load_witness(xi) for xi in x]
        for _ in range(max_path_len):
            node_offset = ctx.mul(node_idx, Constant(5))
            data_slot_idx = ctx.add(node_offset, Constant(0))
            data_slot = ctx.select_from_idx(tree, data_slot_idx)
            x_copy = []
            for i in range(len(x)):
                x_copy.append(ctx.load_witness(x[i]))
                ctx.constrain_equal(x_copy[-1], x_advice[i])
            data = ctx.select_from_idx(x_copy, data_slot)
            split_idx = ctx.add(node_offset, Constant(1))
            split = ctx.select_from_idx(tree, split_idx)
            diff = self.chip.qsub(ctx, data, split)
            is_less = self.chip.is_neg(ctx, diff)
            left_idx_idx = ctx.add(node_offset, Constant(2))
            left_idx = ctx.select_from_idx(tree, left_idx_idx)
            right_idx_idx = ctx.add(node_offset, Constant(3))
            right_idx = ctx.select_from_idx(tree, right_idx_idx)
            node_idx = ctx.select(left_idx, right_idx, is_less)
        offset = ctx.mul(node_idx, Constant(5))
        cls_idx = ctx.add(offset, Constant(4))
        return ctx.select_from_idx(tree, cls_idx)

    def copy_elem(self, ctx, elem):
        return ctx.load_copy(elem)

    def copy_list(self, ctx, x):
        return [self.copy_elem(ctx, x_i) for x_i in x]

    def square(self, ctx, x):
        """x^2 / 2^P of a non-negative quantised cell x"""
        x_square = ctx.mul(x, x)
        num_bits = 2 * PRECISION_BITS + 1
        return self.chip._range(ctx).div_mod(x_square, self.chip.quantization_scale, num_bits * 2)[0]

    def gini(self, ctx, dataset_x, dataset_y, masks, data_slot: int, num_feature: int, num_class: int, split):
        """the weighted Gini impurity, quantised, of splitting the masked samples at feature data_slot < split (a cell)"""
        chip = self.chip
        ctx = chip._range(ctx)
        num_group1 = ctx.load_zero()
        num_group2 = ctx.load_zero()
        targets = zip(list(dataset_x)[data_slot::num_feature], dataset_y, masks)  # (x_ij, y_i, mask_i), j the data slot
        one = Constant(1)
        proportion_cls_grp1 = [ctx.load_zero()] * num_class
        proportion_cls_grp2 = [ctx.load_zero()] * num_class
        cls_adv = [ctx.load_constant(cls_i) for cls_i in range(num_class)]
        cnt = ctx.load_zero()
        for x_ij, y_i, mask_i in targets:
            cnt = ctx.add(cnt, mask_i)
            diff = chip.qsub(ctx, x_ij, split)
            is_less = chip.is_neg(ctx, diff)
            mask_i_copy = self.copy_elem(ctx, mask_i)
            is_less_mask = ctx.mul(is_less, mask_i)
            num_group1 = ctx.add(num_group1, is_less_mask)
            is_greater = ctx.sub(one, is_less)
            is_greater_mask = ctx.mul(is_greater, mask_i_copy)
            num_group2 = ctx.add(num_group2, is_greater_mask)
            for cls_i in range(num_class):
                y_i_copy = self.copy_elem(ctx, y_i)
                is_cls_i = ctx.is_equal(y_i_copy, cls_adv[cls_i])
                is_cls_i_grp1 = ctx.mul(is_cls_i, is_less_mask)
                is_cls_i_grp2 = ctx.mul(is_cls_i, is_greater_mask)
                proportion_cls_grp1[cls_i] = ctx.add(proportion_cls_grp1[cls_i], is_cls_i_grp1)
                proportion_cls_grp2[cls_i] = ctx.add(proportion_cls_grp2[cls_i], is_cls_i_grp2)
        # no sample under the masks: one, so that nothing divides by zero
        cnt_zero = ctx.is_zero(cnt)
        cnt = ctx.select(one, cnt, cnt_zero)
        num_samples = self.copy_elem(ctx, cnt)
        num_bits = 2 * PRECISION_BITS + 1
        scale = Constant(chip.quantization_scale)
        num_group1 = ctx.mul(num_group1, scale)
        num_group1 = ctx.add(num_group1, one)  # a small epsilon: an empty group divides by it
        num_group2 = ctx.mul(num_group2, scale)
        num_group2 = ctx.add(num_group2, one)

        def group(proportions, num_group, count):
            gini_grp = ctx.load_constant(chip.quantization_scale)
            for pi in proportions:
                pi_q = ctx.mul(pi, scale)
                pi_q = ctx.mul(pi_q, scale)
                pi_cls, _ = ctx.div_mod_var(pi_q, num_group, num_bits * 2, num_bits)
                pi_cls_square = self.square(ctx, pi_cls)
                gini_grp = ctx.sub(gini_grp, pi_cls_square)
            weight_grp, _ = ctx.div_mod_var(num_group, count, num_bits * 2, num_bits)
            gini_grp = ctx.mul(gini_grp, weight_grp)
            return ctx.div_mod(gini_grp, chip.quantization_scale, num_bits)[0]  # rescale

        gini_grp1 = group(proportion_cls_grp1, num_group1, cnt)
        gini_grp2 = group(proportion_cls_grp2, num_group2, num_samples)
        gini = ctx.add(gini_grp1, gini_grp2)
        fix_zero = ctx.is_less_than_safe(num_samples, 2)  # a node of one sample or none: the impurity 1.0, which no candidate beats
        return ctx.select(scale, gini, fix_zero)

    def get_split(self, ctx, dataset_x, dataset_y, masks, num_feature: int, num_class: int):
        """(best_slot, best_split): the candidate of the least Gini among every sample x feature whose sample the masks hold, the first
        of equals; slot 0 and dataset_x[0] where no candidate is below 1.0"""
        chip = self.chip
        ctx = chip._range(ctx)
        num_bits = 2 * PRECISION_BITS + 1
        dataset_x, dataset_y, masks = list(dataset_x), list(dataset_y), list(masks)
        dataset_x_copy = self.copy_list(ctx, dataset_x)
        masks_feature = [self.copy_list(ctx, masks) for _ in range(num_feature)]
        masks_copy = [masks_feature[j][i] for i in range(len(dataset_y)) for j in range(num_feature)]
        slots = [j for _ in range(len(dataset_y)) for j in range(num_feature)]
        best_slot = ctx.load_zero()
        best_split = self.copy_elem(ctx, dataset_x[0])
        best_gini = ctx.load_constant(chip.quantization_scale)  # an impurity is at most 0.5
        for slot, split, mask in zip(slots, dataset_x_copy, masks_copy):
            masks_tmp = self.copy_list(ctx, masks)
            for i in range(len(masks_tmp)):
                masks_tmp[i] = ctx.mul(masks_tmp[i], mask)
            dataset_x_tmp = self.copy_list(ctx, dataset_x)
            dataset_y_tmp = self.copy_list(ctx, dataset_y)
            gini = self.gini(ctx, dataset_x_tmp, dataset_y_tmp, masks_tmp, slot, num_feature, num_class, split)
            is_better = ctx.is_less_than(gini, best_gini, num_bits)
            best_gini = ctx.select(gini, best_gini, is_better)
            slot_adv = ctx.load_constant(slot)
            best_slot = ctx.select(slot_adv, best_slot, is_better)
            best_split = ctx.select(split, best_split, is_better)
        return best_slot, best_split

    def common_cls(self, ctx, dataset_y, masks, num_class: int):
        """the most common class among the masked samples, the lowest of equals; 0 for none"""
        ctx = self.chip._range(ctx)
        num_bits = 2 * PRECISION_BITS + 1
        cls, cnt_cls = [], []
        for i in range(num_class):
            cls.append(ctx.load_constant(i))
            cnt_cls.append(ctx.load_zero())
        for yi, mask in zip(dataset_y, masks):
            for i in range(num_class):
                is_cls = ctx.is_equal(yi, cls[i])
                is_cls_mask = ctx.mul(is_cls, mask)
                cnt_cls[i] = ctx.add(cnt_cls[i], is_cls_mask)
        out_cls = ctx.load_zero()
        max_cnt = ctx.load_zero()
        for cls_idx, cnt in enumerate(cnt_cls):
            is_better = ctx.is_less_than(max_cnt, cnt, num_bits)
            max_cnt = ctx.select(cnt, max_cnt, is_better)
            out_cls = ctx.select(cls[cls_idx], out_cls, is_better)
        return out_cls

    def train(self, ctx, dataset_x, dataset_y, num_feature: int, num_class: int, max_depth: int, min_size: int) -> list:
        """a complete binary tree of max_depth layers over the samples, breadth first, as the flat list `inference` takes: a node of
        at most min_size samples is a leaf, every node of the last layer is one"""
        chip = self.chip
        ctx = chip._range(ctx)
        dataset_x, dataset_y = list(dataset_x), list(dataset_y)
        assert len(dataset_x) == len(dataset_y) * num_feature
        assert min_size >= 1
        assert max_depth >= 1
        assert num_class >= 2
        mask_cls = ctx.load_constant(MASK_CLS)
        min_size = ctx.load_constant(min_size + 1)
        num_bits = 2 * PRECISION_BITS + 1
        queue = [[ctx.load_constant(1)] * len(dataset_y)]
        one = ctx.load_constant(1)
        two = ctx.load_constant(2)
        zero = ctx.load_zero()
        tree = []
        idx_list = [ctx.load_constant(i * num_feature) for i in range(len(dataset_y))]
        for layer in range(max_depth):
            for node_idx in range(len(queue)):
                masks = queue.pop(0)
                masks_copy = self.copy_list(ctx, masks)
                cnt_sample = chip.qsum(ctx, masks_copy)
                leaf = ctx.is_less_than(cnt_sample, min_size, num_bits)
                masks_left = self.copy_list(ctx, masks)
                masks_right = self.copy_list(ctx, masks)
                dataset_x_tmp = self.copy_list(ctx, dataset_x)
                dataset_y_tmp = self.copy_list(ctx, dataset_y)
                masks_tmp = self.copy_list(ctx, masks)
                best_slot, best_split = self.get_split(ctx, dataset_x_tmp, dataset_y_tmp, masks_tmp, num_feature, num_class)
                for idx in range(len(dataset_y)):
                    value_idx = ctx.add(best_slot, idx_list[idx])
                    dataset_x_copy = self.copy_list(ctx, dataset_x)
                    value = ctx.select_from_idx(dataset_x_copy, value_idx)
                    diff = chip.qsub(ctx, value, best_split)
                    is_left = chip.is_neg(ctx, diff)
                    masks_left[idx] = ctx.mul(masks_left[idx], is_left)
                    is_right = ctx.not_(is_left)
                    masks_right[idx] = ctx.mul(masks_right[idx], is_right)
                dataset_y_copy = self.copy_list(ctx, dataset_y)
                cls = self.common_cls(ctx, dataset_y_copy, masks, num_class)
                cur_idx = ctx.load_constant(2 ** layer - 1 + node_idx)
                if layer < max_depth - 1:
                    queue.append(masks_left)
                    queue.append(masks_right)
                    cls = ctx.select(cls, mask_cls, leaf)
                    left_child = ctx.mul_add(cur_idx, two, one)
                    right_child = ctx.mul_add(cur_idx, two, two)
                    left_child = ctx.select(cur_idx, left_child, leaf)
                    right_child = ctx.select(cur_idx, right_child, leaf)
                    best_slot = ctx.select(zero, best_slot, leaf)
                    best_split = ctx.select(zero, best_split, leaf)
                    tree.append([best_slot, best_split, left_child, right_child, cls])
                else:  # every node of the last layer is a leaf
                    left_child = self.copy_elem(ctx, cur_idx)
                    tree.append([zero, zero, left_child, cur_idx, cls])
        return [cell for node in tree for cell in node]


# ---- the closures of examples/decision_tree.rs; the sizes are the module's, read when a closure runs, and default to the reference's --------
num_feature = 2
num_class = 2
max_depth = 4
min_size = 1
max_path_len = 3
_q = FixedPointChip(PRECISION_BITS).quantization
# seven nodes: 0 and 1 inner, 2 .. 4 the leaves a path reaches, 5 and 6 padding
tree = [0, _q(1.3), 1, 2, MASK_CLS,
        1, _q(-3.5), 3, 4, MASK_CLS,
        0, 0, 2, 2, 1,
        0, 0, 3, 3, 1,
        0, 0, 4, 4, 0,
        0, 0, 5, 5, 0,
        0, 0, 6, 6, 1]


def inference(ctx, inputs, make_public):
    """inputs: x, quantised.  The class is public; the tree is the module's `tree`, constants of the circuit and so part of the key"""
    chip = DecisionTreeChip(ctx.lookup_bits)
    make_public.append(chip.inference(ctx, tree, list(inputs), max_path_len))


def train(ctx, inputs, make_public):
    """inputs (x, y): x the samples' features, quantised and flat (sample by sample), y their classes.  The tree is public"""
    x, y = inputs
    chip = DecisionTreeChip(ctx.lookup_bits)
    x_deq = [ctx.load_witness(v) for v in x]
    y_adv = [ctx.load_witness(v) for v in y]
    make_public += chip.train(ctx, x_deq, y_adv, num_feature, num_class, max_depth, min_size)


def quantize_dataset(chip: FixedPointChip, x, y):
    """real samples x[sample][feature] and classes y -> the inputs of `train`"""
    return [chip.quantization(v) for xi in x for v in xi], [int(v) for v in y]


def nodes(chip: FixedPointChip, public) -> list:
    """the public outputs of `train` as the reference prints them: a row of floats per node, the split of an inner node dequantised"""
    rows = []
    for at in range(0, len(public), 5):
        node = [float(v) for v in public[at:at + 5]]
        if node[4] == float(MASK_CLS):
            node[1] = chip.dequantization(public[at + 1])
        rows.append(node)
    return rows
