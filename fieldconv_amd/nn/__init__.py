from .tangent_nonlin import TangentNonLin
from .tangent_lin import TangentLin
from .tangent_perceptron import TangentPerceptron
from .trans_field import TransField
from .field_conv import FieldConv
from .echo import ECHO
from .lift_block import LiftBlock
from .fc_resnet_block import FCResNetBlock
from .echo_block import ECHOBlock
from .label_smoothing_loss import LabelSmoothingLoss
from .twin_loss import TwinLoss
from .twin_eval import TwinEval
from .mesh_pool import MeshPool
from .linear_cross_entropy import LinearCrossEntropy
from ..head import vertex_accuracy
from .tangent_pool import TangentPool, TangentUnpool
from .tangent_norm import TangentNorm
from .tangent_interpolate import TangentInterpolate
from .tangent_max_pool import TangentMaxPool
from .mesh_max_pool import MeshMaxPool
from .tangent_dropout import TangentDropout
from .tangent_gradient import TangentDivergence, TangentGradient
from .tangent_diffusion import TangentDiffusion

__all__ = ['TangentNonLin', 'TangentLin', 'TangentPerceptron', 'TransField', 'FieldConv', 'ECHO', 'LiftBlock',
           'FCResNetBlock', 'ECHOBlock', 'LabelSmoothingLoss', 'TwinLoss', 'TwinEval',
           'LinearCrossEntropy', 'vertex_accuracy', 'TangentPool', 'TangentUnpool', 'TangentNorm', 'TangentInterpolate',
           'TangentMaxPool', 'MeshMaxPool', 'TangentDropout', 'TangentGradient', 'TangentDivergence', 'TangentDiffusion', 'MeshPool']
