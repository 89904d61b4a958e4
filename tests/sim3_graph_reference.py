"""The Sim(3) graph queries (tb_kf_store_sim3_graph_dev, tb_vo_loop_sim3_dev) on the CPU: the graph builder from its rules, then
tests/pose_graph_sim3_reference.py's solver.

Per sequence: nodes are the live ring slots in ascending kf_id -- slot (oldest + i) % capacity, which slots are live following
from the store's count alone -- then the query frame; the other nodes up to capacity + 1 are the identity, which no edge names. A
node is the quaternion form of its float32 Tcw (pose_graph_reference.quat_from_R, the kernels' rule) with s = 1; node 0 is
fixed. Odometry edges Z = S_next S_prev^-1 join consecutive nodes; the loop edge has a = the node of best_kf, b = the frame's
node and Z = best_srt byte for byte. best_kf < 0 or fewer than 2 live keyframes: no edge. A best_kf the ring no longer holds:
a = -1, which the solver flags. Every edge slot that is not used is zero."""
import numpy as np

import pose_graph_reference as pg
import pose_graph_sim3_reference as s3

IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0, 1.0])


def node_from_pose(T32):
    T = np.asarray(T32, np.float32).astype(np.float64).reshape(4, 4)
    q = pg.quat_from_R(T[:3, :3])
    return np.array([q[3], q[0], q[1], q[2], T[0, 3], T[1, 3], T[2, 3], 1.0])


def build(Tcw, kf_ids, nadded, q_Tcw, best_kf, best_srt, w=(1.0, 1.0, 1.0), frame_id=-2):
    """Tcw [capacity, 4, 4] float32 and kf_ids [capacity] of one sequence's ring, the store's count, the query pose, the kept
    winner -> dict(nnodes, node_kf [nn], nodes [nn, 8], edges [nn] EDGE, count)"""
    cap = len(kf_ids)
    nn = cap + 1
    nlive = min(int(nadded), cap)
    oldest = int(nadded) % cap if nadded >= cap else 0
    slots = [(oldest + i) % cap for i in range(nlive)]
    nodes = np.tile(IDENTITY, (nn, 1))
    node_kf = np.full(nn, -1, np.int32)
    for i, sl in enumerate(slots):
        nodes[i], node_kf[i] = node_from_pose(Tcw[sl]), kf_ids[sl]
    nodes[nlive], node_kf[nlive] = node_from_pose(q_Tcw), frame_id
    edges = np.zeros(nn, s3.EDGE)
    loop = best_kf >= 0 and nlive >= 2
    if loop:
        for i in range(nlive):
            Z = s3.srt_to_matrix(nodes[i + 1]) @ s3.inv(s3.srt_to_matrix(nodes[i]))
            edges[i] = s3.make_edge(i, i + 1, Z, *w)
            edges[i]["srt"][7] = 1.0
        j = -1
        for i, sl in enumerate(slots):
            if kf_ids[sl] == best_kf:
                j = i
        edges[nlive] = s3.make_edge(0, 0, np.eye(4), *w)
        edges[nlive]["a"], edges[nlive]["b"], edges[nlive]["srt"] = j, nlive, best_srt
    return dict(nnodes=nlive + 1, node_kf=node_kf, nodes=nodes, edges=edges, count=nlive + 1 if loop else 0)


def query(Tcw, kf_ids, nadded, q_Tcw, best_kf, best_srt, iters=10, fixed_scale=True, w=(1.0, 1.0, 1.0), frame_id=-2):
    """build, then the solver on the capacity + 1 nodes with node 0 fixed: build's dict plus after [nn, 8] and stats [8]"""
    g = build(Tcw, kf_ids, nadded, q_Tcw, best_kf, best_srt, w, frame_id)
    g["after"], g["stats"] = s3.solve(g["nodes"], 1, g["edges"][:g["count"]], iters, fixed_scale)
    return g
