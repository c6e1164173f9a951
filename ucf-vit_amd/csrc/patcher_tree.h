// The tree of the adaptive patcher, shared by its builders (quadtree.hip) and by the kernels that read (nodes, count) back
// (patcher_labels.hip): the node, the decoded leaf, the greedy refinement of the reference's FixedQuadTree / FixedOctTree
// (dataloaders/quadtree.py:115-140, octree.py:73-110) for ND = 2, 3, its output loop, and the index decode of a leaf's outputs.
// Integer logic only: nothing here depends on how a translation unit contracts floating-point expressions.
#pragma once

// a box [c[0], c[1]) x [c[2], c[3]) [x [c[4], c[5])] = x1, x2, y1, y2[, z1, z2] and its value.  The builders' LDS node lists, and with them
// the accepted fixed_length, follow from these sizes.
template <int ND>
struct Node {
    short c[2 * ND];
    int v;
};
static_assert(sizeof(Node<2>) == 12 && sizeof(Node<3>) == 16, "the LDS node lists are sized for 12- and 16-byte nodes");

// one row of nodes int32 [B][L][2 ND], decoded: origin and extent per axis (0 = x, 1 = y, 2 = z)
template <int ND>
struct Leaf {
    int o[ND], n[ND];
    __device__ __forceinline__ explicit Leaf(const int* __restrict__ q) {
#pragma unroll
        for (int a = 0; a < ND; ++a) {
            o[a] = q[2 * a];
            n[a] = q[2 * a + 1] - q[2 * a];
        }
    }
    __device__ __forceinline__ bool empty() const {
        bool e = false;
#pragma unroll
        for (int a = 0; a < ND; ++a) e = e || n[a] <= 0;
        return e;
    }
    // the box lies in an image of dims[a] pixels along axis a
    __device__ __forceinline__ bool inside(const int (&dims)[ND]) const {
        bool in = true;
#pragma unroll
        for (int a = 0; a < ND; ++a) in = in && o[a] >= 0 && o[a] + n[a] <= dims[a];
        return in;
    }
};

// The greedy refinement, by one workgroup of 256 threads: starting from `root`, replace the FIRST node of maximum value by its 2^ND children,
// in place, until L nodes exist or that node is 2 wide in x.  cur / nxt: two LDS lists of L + 2^ND nodes; value(node) is the region-sum rule.
// Returns the number of nodes and leaves `cur` pointing at the list that holds them.
template <int ND, typename Value>
__device__ __forceinline__ int tree_refine(Node<ND>*& cur, Node<ND>* nxt, int L, Node<ND> root, Value value) {
    constexpr int K = 1 << ND;
    __shared__ int red_v[4], red_i[4];
    __shared__ int s_idx, s_stop;
    __shared__ Node<ND> s_kids[K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nt = blockDim.x;          // read once: left in the loops, the load of the workgroup size is repeated in every refinement step
    int n = 1;
    if (tid == 0) {
        root.v = value(root);
        cur[0] = root;
        s_stop = 0;
    }
    __syncthreads();
    while (n < L) {
        // first index of the maximum value: max over (v, -i)
        int bv = -1, bi = 0x7fffffff;
        for (int i = tid; i < n; i += nt) {
            const int v = cur[i].v;
            if (v > bv) {          // i ascends per thread: the first maximum of this thread's subsequence is kept
                bv = v;
                bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const int ov = __shfl_xor(bv, o, 64), oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            red_v[wave] = bv;
            red_i[wave] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            int v = red_v[0], i = red_i[0];
            for (int w = 1; w < 4; ++w)
                if (red_v[w] > v || (red_v[w] == v && red_i[w] < i)) {
                    v = red_v[w];
                    i = red_i[w];
                }
            s_idx = i;
            if (cur[i].c[1] - cur[i].c[0] == 2) s_stop = 1;            // quadtree.py:121-122, octree.py:79-80
        }
        __syncthreads();
        if (s_stop) break;
        const int idx = s_idx;
        if (tid < K) {
            // child tid takes the upper half of axis a when bit a of tid is set (octree.py:83-103: n1..n8, x fastest, then y, then z); the
            // quadtree's lt, rt, lb, rb (quadtree.py:125) is the same rule with the y bit inverted
            const Node<ND> q = cur[idx];
            Node<ND> k;
#pragma unroll
            for (int a = 0; a < ND; ++a) {
                const short lo = q.c[2 * a], hi = q.c[2 * a + 1];
                const short mid = (short)((lo + hi) >> 1);                  // int((a + b) / 2) for non-negative ints
                const bool upper = (((tid >> a) & 1) != 0) != (ND == 2 && a == 1);
                k.c[2 * a] = upper ? mid : lo;
                k.c[2 * a + 1] = upper ? hi : mid;
            }
            k.v = value(k);
            s_kids[tid] = k;
        }
        __syncthreads();
        // nodes = nodes[:idx] + kids + nodes[idx+1:]   (quadtree.py:134), written into the other list
        for (int j = tid; j < n + K - 1; j += nt) nxt[j] = j < idx ? cur[j] : (j < idx + K ? s_kids[j - idx] : cur[j - (K - 1)]);
        __syncthreads();
        Node<ND>* t = cur;
        cur = nxt;
        nxt = t;
        n += K - 1;
    }
    return n;
}

// Outputs of image b: the first min(n, L) nodes (n == L whenever fixed_length = (2^ND - 1) k + 1), their values, seq_ps = (width, centre per
// axis) and the count; the rows behind them padded as the reference's serialize() pads (quadtree.py:160-168)
template <int ND>
__device__ __forceinline__ void tree_write(const Node<ND>* cur, int n, int L, int b, int* __restrict__ nodes_out, int* __restrict__ values_out,
                                           int* __restrict__ count_out, float* __restrict__ seq_ps) {
    const int nv = n < L ? n : L;
    if (threadIdx.x == 0) count_out[b] = nv;
    for (int i = threadIdx.x; i < L; i += blockDim.x) {
        int* no = nodes_out + ((int64_t)b * L + i) * (2 * ND);
        float* sp = seq_ps + ((int64_t)b * L + i) * (ND + 1);
        if (i < nv) {
            const Node<ND> q = cur[i];
#pragma unroll
            for (int k = 0; k < 2 * ND; ++k) no[k] = q.c[k];
            values_out[(int64_t)b * L + i] = q.v;
            sp[0] = (float)(q.c[1] - q.c[0]);                                  // seq_size: the width (quadtree.py:151)
#pragma unroll
            for (int a = 0; a < ND; ++a) sp[1 + a] = (float)(q.c[2 * a + 1] + q.c[2 * a]) * 0.5f;      // seq_pos: centre (:152, Rect.get_center)
        } else {
#pragma unroll
            for (int k = 0; k < 2 * ND; ++k) no[k] = 0;
            values_out[(int64_t)b * L + i] = 0;
            sp[0] = 0.f;
#pragma unroll
            for (int a = 0; a < ND; ++a) sp[1 + a] = -1.f;
        }
    }
}

// (c, x[0..ND)) of output number i of a leaf of extents n: x fastest, then y (, z), then c (planar outputs) or c fastest, then x, y (, z)
// (channels-last outputs), so that consecutive lanes write consecutive addresses.  I: unsigned where the leaf has fewer than 2^31 outputs,
// else int64_t.
template <int ND, typename I>
__device__ __forceinline__ void leaf_index(I i, int C, const int (&n)[ND], int c_fast, int& c, int (&x)[ND]) {
    I r = i;
    if (c_fast) {
        c = (int)(r % (I)C);
        r /= (I)C;
    }
#pragma unroll
    for (int a = 0; a < ND - 1; ++a) {
        x[a] = (int)(r % (I)n[a]);
        r /= (I)n[a];
    }
    if (c_fast) {
        x[ND - 1] = (int)r;
    } else {
        x[ND - 1] = (int)(r % (I)n[ND - 1]);
        c = (int)(r / (I)n[ND - 1]);
    }
}
