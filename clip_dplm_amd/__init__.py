"""clip_dplm_amd — MI355X-native (gfx950) CLIP-style dual-encoder contrastive path of SrikarK-code/clip-dplm.

Python mirrors of the reference's module API on top of libclipk.so (hand-written HIP kernels behind the C ABI
in include/clipk.h).  There is no CPU fallback: every forward needs device tensors and the built library.
"""
from .configuration_hybrid_clip import HybridCLIPConfig, ModelArchitectureConfig, SubConfig, TrainingConfig
from .encoders import ESM2Encoder, ESM2_SHAPES, TransformerSeqEncoder, pool
from .esm_integration import (BiologicalDataType, ESMConfig, ESMIntegration, ESMOutput, GeneProjection,
                              ProteinProjection, create_esm_integration, get_embeddings_batch)
from .data import MemoryQueue
from .functional import set_linear_precision
from .loss import clip_loss, contrastive_loss
from .modeling_clip import (CLIPEncoder, DiffMapProteinCLIP, DiffMapProteinCLIPModule, OptimizedCLIPModule,
                            OptimizedProjectionHead, ProjectionHead, RNAProteinCLIP, RNAProteinCLIPModule,
                            optimized_clip_loss)
from .modeling_seqclip import (ProteinRNACLIP, RNARBPCLIPEncoder, RNARBPCLIPModel, RNARBPCLIPProjectionHead,
                               create_padding_mask)
from .modeling_trimodal import CellStateEncoder, ContrastiveModel, PerturbationEncoder, TransformerEncoder
from .optim import FlatParams, FusedAdamW, cosine_annealing_lr
from .training import (CosineAnnealingLR, EarlyStopping, GraphedTrainStep, evaluate_model, load_checkpoint, save_checkpoint,
                       train_epoch)
from . import training
from .retrieval import EmbeddingIndex, evaluate_retrieval, metrics_from_ranks, retrieval_metrics
from . import retrieval
from .diagnostics import SimilarityStats, evaluate_embeddings, similarity_stats
from . import diagnostics
from .classifier import LinearClassifier, MLPClassifier, SimpleNonLinearClassifier, TransformerClassifier
from . import classifier, probe
from .ot import SinkhornResult, sinkhorn, sinkhorn_divergence
from .ot import AssignmentResult, exact_assignment, wasserstein2_exact
from . import ot
from .flow import SchrodingerBridgeConditionalFlowMatcher, conditional_flow, flow_matching_loss
from .flow import ExactOptimalTransportConditionalFlowMatcher, linear_conditional_flow
from . import flow
from .distribution import evaluate_distributions, frechet_distance, mmd2
from . import distribution
from .cluster import (KMeansResult, adjusted_rand_index, cluster_agreement, contingency, kmeans,
                      normalized_mutual_info)
from .cluster import (calinski_harabasz_score, choose_n_clusters, davies_bouldin_score, label_separation,
                      silhouette_by_label, silhouette_samples, silhouette_score)
from . import cluster
from .manifold import TSNEResult, embed_spaces, knn_preservation, perplexity_bandwidths, tsne
from . import manifold
from .mixing import LabelMasses, integration_scores, label_masses, label_transfer, label_transfer_accuracy, lisi
from .mixing import KBETResult, kbet, lisi_knn
from . import mixing
from .neighbors import KNNGraph, knn_graph
from . import neighbors
from .diffusion import DiffusionMap, SymGraph, connectivities, diffusion_map, dpt, pseudotime, pseudotime_preservation
from . import diffusion
from .paga import PAGAPreservation, PAGAResult, connectivities_tree, group_edge_counts, modularity, paga_preservation
from . import paga              # the module: its function of the same name is paga.paga

__all__ = [
    "HybridCLIPConfig", "ModelArchitectureConfig", "TrainingConfig", "SubConfig",
    "CLIPEncoder", "ProjectionHead", "RNAProteinCLIPModule", "DiffMapProteinCLIPModule", "RNAProteinCLIP",
    "DiffMapProteinCLIP", "OptimizedProjectionHead", "OptimizedCLIPModule", "optimized_clip_loss",
    "RNARBPCLIPProjectionHead", "RNARBPCLIPEncoder", "RNARBPCLIPModel", "create_padding_mask", "ProteinRNACLIP",
    "ContrastiveModel", "CellStateEncoder", "PerturbationEncoder", "TransformerEncoder",
    "ESM2Encoder", "ESM2_SHAPES", "TransformerSeqEncoder", "pool", "clip_loss", "FlatParams", "FusedAdamW",
    "cosine_annealing_lr", "CosineAnnealingLR", "GraphedTrainStep", "EarlyStopping", "train_epoch", "evaluate_model", "save_checkpoint",
    "load_checkpoint", "ESMConfig", "ESMIntegration", "ESMOutput", "BiologicalDataType", "ProteinProjection",
    "GeneProjection", "create_esm_integration", "get_embeddings_batch", "MemoryQueue", "contrastive_loss", "set_linear_precision",
    "retrieval", "EmbeddingIndex", "evaluate_retrieval", "retrieval_metrics", "metrics_from_ranks",
    "diagnostics", "SimilarityStats", "similarity_stats", "evaluate_embeddings",
    "classifier", "probe", "MLPClassifier", "TransformerClassifier", "LinearClassifier", "SimpleNonLinearClassifier",
    "ot", "sinkhorn", "sinkhorn_divergence", "SinkhornResult",
    "flow", "SchrodingerBridgeConditionalFlowMatcher", "conditional_flow", "flow_matching_loss",
    "AssignmentResult", "exact_assignment", "wasserstein2_exact",
    "ExactOptimalTransportConditionalFlowMatcher", "linear_conditional_flow",
    "distribution", "mmd2", "frechet_distance", "evaluate_distributions",
    "cluster", "kmeans", "KMeansResult", "contingency", "adjusted_rand_index", "normalized_mutual_info",
    "cluster_agreement", "silhouette_samples", "silhouette_score", "silhouette_by_label", "davies_bouldin_score",
    "calinski_harabasz_score", "label_separation", "choose_n_clusters",
    "manifold", "tsne", "TSNEResult", "perplexity_bandwidths", "embed_spaces", "knn_preservation",
    "mixing", "lisi", "label_masses", "LabelMasses", "label_transfer", "label_transfer_accuracy", "integration_scores",
    "kbet", "KBETResult", "lisi_knn", "neighbors", "knn_graph", "KNNGraph",
    "diffusion", "connectivities", "diffusion_map", "pseudotime", "dpt", "pseudotime_preservation", "SymGraph", "DiffusionMap",
    "paga", "group_edge_counts", "connectivities_tree", "modularity", "paga_preservation", "PAGAResult", "PAGAPreservation",
]
