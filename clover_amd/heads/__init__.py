from .mlm_itm_head import ITMHead, MLMHead
from .qa_head import QA_MC_head, QA_OE_Head
from .ssl_head import NCEHeadForMM, NCEHeadForText, NCEHeadForVision

__all__ = ['NCEHeadForMM', 'NCEHeadForText', 'NCEHeadForVision', 'MLMHead', 'ITMHead', 'QA_MC_head', 'QA_OE_Head']
