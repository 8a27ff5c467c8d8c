"""dl_vqa_amd — the VqaNet train-step hot path of OmerShubi/DL_VQA on MI355X (gfx950).

``VqaNet`` is a drop-in ``torch.nn.Module`` (reference models/model.py:7-67) whose forward and
backward run on hand-written HIP kernels (csrc/, bound through the C ABI in include/vqa_hip.h);
``train`` mirrors the reference training procedure (train.py) with a fused device-side loss and
Adam; ``distributed.DataParallel`` shards the minibatch over the GPUs of one node with RCCL.
``VqaNet.encode_images`` / ``answer`` (inference) and ``VqaNet.forward_shared`` / ``train.run_batch_shared`` (training)
serve batches in which several questions ask about the same image: the image-only work runs once per image.
``topk_answers`` / ``VqaNet.predict`` rank the answers on the device -- the k best per question with their probabilities, in
the order the VQA score's arg-max uses -- and return them as ``TopAnswers``.
``VqaNet.encode_questions`` / ``answer_pairs`` / ``predict_pairs`` are the mirror image of the image cache: every distinct
question is encoded once (``unique_questions`` deduplicates a batch) and (image, question) pairs are answered from the two caches.
``VqaNet.forward_features`` / ``train.run_batch_features`` train the question encoder, the attention stage and the classifier on
cached image features (``encode_images(v, with_vprime=False)``, ``ImageFeatures.cat``) with the image encoder frozen: no
convolution runs in the step, and only the bank rows a batch asks about are touched (``compact_image_index``).
``preprocess_images`` turns decoded RGB images of any sizes into the ``v [N,3,S,S]`` all of these start from -- the reference's
resize, centre crop, normalisation and fp16 cast (preprocessing/preprocess_images.py), bit for bit, in one kernel launch.
``VqaNet.explain`` / ``explain_pairs`` are ``answer`` / ``answer_pairs`` with a gradient x input map per question
(``Attribution``): why an answer, at the normalised feature layer, from the same caches and without a convolution.
``VqaNet.explain_words`` carries the same gradient on to the question: one gradient x input value per token
(``WordAttribution``), back through q_lin, the attention scores and the LSTM, with no parameter gradient formed.
``VqaNet.explain_occlusion`` / ``explain_occlusion_pairs`` return what those maps estimate, exactly (``Occlusion``): how far
the logit falls when a window of grid positions is taken out of the image, for every position, in closed form.
``VqaNet.explain_words_occlusion`` does the same for the question (``WordOcclusion``): how far the logit falls when one token's
embedding output is zeroed, for every token, from the prefixes the variant recurrences share with the question itself.
``VqaNet.explain_faithfulness`` / ``explain_faithfulness_pairs`` say how well any such map ranks the grid positions
(``Faithfulness``): the deletion and insertion curves of the explained logit along the map's ranking, and their areas.
``VqaNet.explain_integrated`` / ``explain_integrated_pairs`` repair the first-order map (``IntegratedGradients``): the same
gradient averaged along the path from a cache of zeros to the real one, which sums to the logit's rise over that baseline;
v' is read twice whatever the number of steps.
``VqaNet.explain_shapley`` / ``explain_shapley_pairs`` give the sampled Shapley value of every grid position (``Shapley``) for
the set function those curves walk, with a standard error per entry, from orders drawn by ``shapley_orders``.
``VqaNet.explain_faithfulness_probs`` / ``explain_faithfulness_probs_pairs`` walk the same curves on probabilities
(``ProbabilityCurves``): the softmax probability of the explained column and the arg-max column at every step, the published
deletion / insertion areas, and the steps at which the answer flips.
"""
from .model import VqaNet, questionNet, ImageNet2, Attention, Classifier, ImageFeatures, group_by_image, TopAnswers, topk_answers, QuestionFeatures, unique_questions, compact_image_index, Attribution, WordAttribution, Occlusion, WordOcclusion, Faithfulness, IntegratedGradients, Shapley, shapley_orders, ProbabilityCurves  # noqa: F401
from .preprocess import preprocess_images  # noqa: F401

__all__ = ["VqaNet", "questionNet", "ImageNet2", "Attention", "Classifier", "ImageFeatures", "group_by_image", "TopAnswers",
           "topk_answers", "QuestionFeatures", "unique_questions", "preprocess_images", "compact_image_index", "Attribution",
           "WordAttribution", "Occlusion", "WordOcclusion", "Faithfulness", "IntegratedGradients", "Shapley",
           "shapley_orders", "ProbabilityCurves"]
